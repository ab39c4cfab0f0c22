"""The one reader of the gfx950 code object INSIDE the built library (no second compile): libhades252.so's .hip_fatbin is
unbundled once per process and library file, its AMDGPU metadata note read, and -- only when a test asks for a kernel's
body -- disassembled once.  Kernels are selected by their exact function name, never by a substring of the mangled one."""
import functools
import logging
import os
import re
import subprocess
import tempfile

import pytest

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
log = logging.getLogger(__name__)


def _tools(*names):
    paths = [os.path.join(LLVM, t) for t in names]
    if not all(os.path.exists(t) for t in paths):
        pytest.skip("ROCm LLVM tools not available")
    return paths


def function_name(mangled):
    """The function's own name from the Itanium length prefixes: _Z16k_witness_cipherILb0EE... -> k_witness_cipher,
    _ZN5hades11k_perm_fastE... -> k_perm_fast (the last component of a nested name)."""
    head = re.match(r"_Z(N?)", mangled)
    if head is None:
        return mangled                                               # extern "C"
    pos, name = head.end(), None
    while True:
        length = re.compile(r"\d+").match(mangled, pos)
        if length is None:
            return name
        pos = length.end() + int(length.group())
        name = mangled[length.end():pos]
        if not head.group(1):                                        # not nested: what follows are the parameters
            return name


def mads(body):
    """The 64-bit multiply-adds of a disassembled kernel: what the field arithmetic is made of."""
    return len(re.findall(r"\bv_mad_[iu]64_[iu]32\b", body))


class CodeObject:
    """`meta[mangled name]`: every integer field of the kernel's amdhsa.kernels entry; `body(mangled name)`: its
    disassembly; `kernels(base)`: the mangled names of the kernels whose function name is `base`."""

    def __init__(self, lib_path):
        objcopy, bundler, readelf = _tools("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")
        log.info("unbundling %s", lib_path)
        with tempfile.TemporaryDirectory() as tmp:
            fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
            subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, lib_path, os.path.join(tmp, "scratch.so")],
                           check=True)
            subprocess.run([bundler, "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co],
                           check=True)
            notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
            with open(co, "rb") as f:
                self._image = f.read()
        self.meta = {}
        for entry in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:          # one entry of amdhsa.kernels per kernel
            m = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
            if m is not None:                                                    # keys of the entry itself, not of its .args
                self.meta[m.group(1)] = {k: int(v) for k, v in re.findall(r"^(?:    )?\.(\w+):\s+(\d+)$", entry, re.M)}

    def kernels(self, base):
        return sorted(k for k in self.meta if function_name(k) == base)

    @functools.cached_property
    def _bodies(self):
        (objdump,) = _tools("llvm-objdump")
        log.info("disassembling the code object")
        with tempfile.TemporaryDirectory() as tmp:
            co = os.path.join(tmp, "gfx950.co")
            with open(co, "wb") as f:
                f.write(self._image)
            text = subprocess.run([objdump, "-d", co], check=True, capture_output=True, text=True).stdout
        parts = re.split(r"^[0-9a-f]+ <(\S+)>:$", text, flags=re.M)
        return {parts[i]: parts[i + 1] for i in range(1, len(parts), 2)}

    def body(self, name):
        return self._bodies[name]


@functools.lru_cache(maxsize=None)
def _load(lib_path, size, mtime_ns):
    return CodeObject(lib_path)


def load(lib_path=None):
    """The code object of the library (default: the built one), read once per process and library file."""
    if lib_path is None:
        from hades252_amd import _lib
        lib_path = _lib.LIB_PATH
    st = os.stat(lib_path)
    return _load(os.path.abspath(lib_path), st.st_size, st.st_mtime_ns)


def assert_perm_witness_budget(co, names, vgpr_cap=152, sgpr_spill_cap=8):
    """Each kernel of `names` has k_perm_witness's budget: its multiply-adds within 2 % of k_perm_witness's in the same
    library (ONE call site of the round loop), no scratch, no spilled VGPR, at most `vgpr_cap` registers (VGPRs + AGPRs:
    one file) and `sgpr_spill_cap` spilled SGPRs."""
    (perm,) = co.kernels("k_perm_witness")
    ref = mads(co.body(perm))
    for name in names:
        n, r = mads(co.body(name)), co.meta[name]
        assert abs(n - ref) <= 0.02 * ref, (name, n, ref)
        assert "scratch_" not in co.body(name)
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] + r["agpr_count"] <= vgpr_cap and r["sgpr_spill_count"] <= sgpr_spill_cap, (name, r)
