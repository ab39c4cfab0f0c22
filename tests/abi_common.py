"""The boundary harness shared by the CPU-tier tests/test_*_abi.py files: what every family asserts about its C entry
points, its section of include/hades252.h, its C++ wrappers and the counter records, with the family's own lists passed in."""
import ctypes
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hades252_amd", "csrc")
INVALID = -1

# fake, never dereferenced: a call that gets them must be refused by the argument checks (or be a no-op success)
PTR = 0x10000          # 16-byte aligned
MIS = PTR + 8          # misaligned


def limbs4(a=1, b=2, c=3, d=4):
    """A scalar as the entry points take it by pointer (a tag, a domain, a capacity): uint64[4]."""
    return (ctypes.c_uint64 * 4)(a, b, c, d)


def header():
    with open(os.path.join(ROOT, "include", "hades252.h")) as f:
        return f.read()


def assert_declared_bound_exported(names):
    """Each name has a prototype in include/hades252.h (comments aside), a ctypes signature in _lib and is exported."""
    from hades252_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in names:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(raw, s), s


def header_block(start_phrase, end_phrase, needles):
    """The header's text from `start_phrase` up to `end_phrase`, which must hold every needle."""
    text = header()
    block = text[text.index(start_phrase):text.index(end_phrase)]
    for needle in needles:
        assert needle in block, needle
    return block


def compile_and_run(tmp_path, name, source, run=True):
    """Compile `source` against include/hades252.hpp with warnings as errors, link it to the built library and (run) run
    it: its stdout lines.  run=False is for snippets that would touch a device: those only have to link."""
    src, exe = tmp_path / (name + ".cpp"), tmp_path / name
    src.write_text(source)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", CSRC,
                    "-lhades252", "-Wl,-rpath," + CSRC, "-o", str(exe)], check=True)
    assert exe.exists()
    if run:
        return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()


def assert_outside_counter_records(files, also_in_deps=()):
    """`files` (kernel sources of a family) are built into the library but define and launch no kernel of a committed
    counter record: they are in UNRECORDED_KERNEL_DEPS and DEPS (as are `also_in_deps`, host-side sources, in DEPS), in
    none of DEVICE_DEPS, LAUNCH_POLICY_DEPS, PERM_FAST_DEPS, and the keys of profiles/hbm_traffic.json are today's
    hashes -- so bench.py keeps replaying its counter-backed traffic."""
    from hades252_amd import build
    files, every = set(files), set(files) | set(also_in_deps)
    assert files <= set(build.UNRECORDED_KERNEL_DEPS) and every <= set(build.DEPS)
    assert not every & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.PERM_FAST_DEPS)
    with open(os.path.join(ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1
