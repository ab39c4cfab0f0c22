"""Build and drive tests/hostsim: the shipped device sources, launch policy and device-pointer C ABI of hades252_amd/csrc
compiled for the CPU and run under the host sanitizers (tests/test_hostsim_*.py).  Test infrastructure only, in the style
of tests/units_lib.py: the product does not link to any of it.

The sources are never edited.  A build works on a temporary copy under tests/hostsim/build/ (git-ignored) to which the
REWRITES below -- an explicit allow-list, each semantically empty on the host -- are applied; it FAILS if an `asm`
statement survives them or if the sources use a `__builtin_amdgcn_*` the stand-in header does not define, so a kernel
edit that adds a new fence or builtin breaks the build instead of being skipped.  MUTANTS are one-line edits of that same
copy with which tests/test_hostsim_mutants.py proves that each detector is live.

Executables, not shared libraries: a sanitized library cannot be loaded into Python without preloading the sanitizer
runtime.  Each run is a subprocess with a timeout, so a deadlocked emulation is a failed test."""
import fcntl
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

from hades252_amd import build as hb

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
HOSTSIM = os.path.join(TESTS, "hostsim")
BUILD = os.path.join(HOSTSIM, "build")
MAIN = os.path.join(HOSTSIM, "hostsim_main.cpp")
STANDIN = os.path.join(HOSTSIM, "hip", "hip_runtime.h")
CLANG = os.environ.get("HOSTSIM_CXX", "/opt/rocm/lib/llvm/bin/clang++")

# the files of the tree that the host build compiles (relative to the repository root); the copy keeps the layout
COPIED = sorted(os.path.join("hades252_amd", "csrc", f) for f in os.listdir(hb.CSRC)
                if f.endswith((".hpp", ".inc"))) + [os.path.join("include", "hades252.h"),
                                                    os.path.join("tests", "units", "arith_units.hip")]

# name -> (pattern, replacement, why it is empty on the host)
REWRITES = {
    # An asm statement with an EMPTY template emits no instruction on any target; its "v" / "s" operand constraints name
    # gfx950 register classes and only pin values for hipcc's optimiser (the comments at each site say so).
    "empty_asm": (re.compile(r'asm volatile\(""\s*:[^;]*\);'), ";"),
    # The dynamic LDS of a launch: on the device an unsized extern array at LDS offset 0, here a pointer to the window the
    # emulator hands out (sized by the launch, the rest poisoned).  Same object for every thread of the block.
    "dynamic_lds": (re.compile(r"extern __shared__ __attribute__\(\(aligned\(16\)\)\) uint8_t lds\[\];"),
                    "uint8_t *const lds = hostsim::dynamic_lds();"),
    # k_witness_duplex keeps one walk per WAVE in LDS (parked_slot): every lane reads it, advances its copy and stores the
    # same value back, with no barrier -- on gfx950 a wave executes each of these LDS instructions for all 64 lanes at once
    # (and the LDS unit serves a wave's requests in order), so every lane reads before any lane writes.  OS threads have no
    # such lockstep: the two rewrites give the emulator that wave-level ordering -- all lanes have read before the store, all
    # have stored before the next read.  No effect on a machine that runs the wave in lockstep.
    "wave_lockstep_store": (re.compile(r"^(\s*)parked_slot\[wave \+ z\] = slot;", re.M),
                            r"\1hostsim::wave_barrier(); parked_slot[wave + z] = slot; hostsim::wave_barrier();"),
    # lanes_perm / rows_perm end with every lane reading a word of the wave's io area (lanes without a word of their own read
    # word 0) and begin with lanes 0..4 / 0..19 storing their input word there.  In a chain kernel (sponge, cipher, duplex
    # sponge: one permutation after another in one wave) nothing but program order lies between that read and the next
    # permutation's store: on gfx950 a wave issues the read for all 64 lanes before the later store instruction and the LDS
    # unit serves a wave's requests in order.  OS threads have no such lockstep, so the emulator gets the wave-level order as
    # a barrier in front of the store (found by TSan on k_sponge_lanes<true>).  No effect on a machine that runs the wave in
    # lockstep.
    "wave_lockstep_input": (re.compile(r"^    if \(lane < (5|20)\) \{$", re.M),
                            r"    hostsim::wave_barrier(); if (lane < \1) {"),
}

FLAGS = {
    "asan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "tsan": ["-O1", "-g", "-fsanitize=thread"],
}
# The driver's table in four executables that compile side by side (HOSTSIM_PART in hostsim_main.cpp): the whole unit
# under ASan+UBSan takes about four minutes to compile, its parts 40 to 100 s each.
PARTS = {"perm": 1, "merkle": 2, "sponge": 4, "witness": 8}
COMMON = ["-x", "c++", "-std=c++17", "-pthread", "-Wno-unused-function", "-Wno-unused-value"]

# name -> (file relative to the root, exact text, replacement), or a list of such edits that belong together: each must
# match exactly once in the rewritten copy
MUTANTS = {
    # ASan: the ragged tail of a store runs one 16-byte chunk past an exact-size buffer
    "store_off_by_one": (os.path.join("hades252_amd", "csrc", "staging.hpp"),
                         "        if (chunk0 + c < total_chunks) g[c] = v;\n    }\n    __syncthreads();\n}\n\n}  // namespace hades",
                         "        if (chunk0 + c <= total_chunks) g[c] = v;\n    }\n    __syncthreads();\n}\n\n}  // namespace hades"),
    # ASan: the launch of k_perm_fast asks for half the LDS its waves use
    "lds_halved": (os.path.join("hades252_amd", "csrc", "launch.hpp"),
                   "hipLaunchKernelGGL(k_perm_fast, dim3(blocks_for(n)), dim3(kBlock), lds_for(5), s, in, out, n);",
                   "hipLaunchKernelGGL(k_perm_fast, dim3(blocks_for(n)), dim3(kBlock), lds_for(5) / 2, s, in, out, n);"),
    # TSan: the transposed read of the slab is no longer ordered after the other lanes' writes
    "load_barrier_removed": (os.path.join("hades252_amd", "csrc", "staging.hpp"),
                             "        *reinterpret_cast<uint4 *>(slab + rec * kLdsRecBytes + part * 16) = v;\n    }\n    __syncthreads();\n",
                             "        *reinterpret_cast<uint4 *>(slab + rec * kLdsRecBytes + part * 16) = v;\n    }\n"),
    # oracle mismatch: the reduction of mont_fips takes the wrong limb of -p (index kept in bounds)
    "negp_index": (os.path.join("hades252_amd", "csrc", "hades_fast.hpp"),
                   "            for (int i = lo; i <= hi; i++) mac(acc, a.l[i], b[k - i]);\n        }\n#pragma unroll\n"
                   "        for (int i = lo; i <= hi; i++)\n            if (k - i >= 1) mac(acc, m[i], NEGP29[k - i]);",
                   "            for (int i = lo; i <= hi; i++) mac(acc, a.l[i], b[k - i]);\n        }\n#pragma unroll\n"
                   "        for (int i = lo; i <= hi; i++)\n            if (k - i >= 1) mac(acc, m[i], NEGP29[k - i - 1]);"),
    # UBSan: a squaring counts the already doubled cross products twice, so a column of maximal lazy limbs (9 * 4.5 * 2^58
    # instead of 9 * 2.25 * 2^58) leaves its 63 bits
    "double_doubled": (os.path.join("hades252_amd", "csrc", "hades_fast.hpp"),
                       "                if (i < j) mac(acc, a.l[i], d[j]);",
                       "                if (i < j) { mac(acc, a.l[i], d[j]); mac(acc, a.l[i], d[j]); }"),
    # TSan: both sides of the helper protocol of the helped one-state-per-wave form use ONE exchange buffer instead of the
    # ping-pong pair, so a main wave publishes round r + 1 while the helper may still be reading round r (hades_lanes.hpp,
    # the comment of LanesLds::xw)
    "xw_single_buffer": [(os.path.join("hades252_amd", "csrc", "hades_lanes.hpp"),
                          "        uint32_t (&xw)[16][8] = L.xw[HELPED ? par : 0];",
                          "        uint32_t (&xw)[16][8] = L.xw[HELPED ? par * 0 : 0];"),
                         (os.path.join("hades252_amd", "csrc", "hades_lanes.hpp"),
                          "        uint32_t (&xw)[16][8] = L.xw[i < 4 ? (i & 1) : ((i + 1) & 1)];",
                          "        uint32_t (&xw)[16][8] = L.xw[0 * i];")],
    # oracle mismatch: the light carry pass of the lane form's linear layer takes the carry one bit too high; every value
    # stays inside its machine word, so no sanitizer has anything to see
    "carry_light_shift": (os.path.join("hades252_amd", "csrc", "hades_lanes.hpp"),
                          "    const uint32_t h = t >> kLB;\n    c16 = h;",
                          "    const uint32_t h = t >> (kLB + 1);\n    c16 = h;"),
    # ASan: lane w of a state wave addresses word w + 1 of its state, so word 4 of the LAST state lies behind the buffer
    "lanes_word_off_by_one": (os.path.join("hades252_amd", "csrc", "kernels_perm.hpp"),
                              "    uint8_t *mine = states + rec * 160 + (lane < 5 ? lane : 0) * 32;\n"
                              "    const Fr in = lane < 5 ? load_word(mine) : zero_word();\n"
                              "    const Fr out = lanes_perm<HELPED>",
                              "    uint8_t *mine = states + rec * 160 + (lane < 5 ? lane + 1 : 0) * 32;\n"
                              "    const Fr in = lane < 5 ? load_word(mine) : zero_word();\n"
                              "    const Fr out = lanes_perm<HELPED>"),
}


def mutant_edits(name) -> list:
    m = MUTANTS[name]
    return list(m) if isinstance(m, list) else [m]


def _strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def standin_builtins() -> set:
    with open(STANDIN) as f:
        return set(re.findall(r"^#define (__builtin_amdgcn_\w+)", f.read(), flags=re.M))


def rewritten(rel: str, mutant=None) -> str:
    """The text of tree file `rel` as the host build compiles it."""
    with open(os.path.join(ROOT, rel)) as f:
        text = f.read()
    for pattern, repl in REWRITES.values():
        text = pattern.sub(repl, text)
    for where, old, new in (mutant_edits(mutant) if mutant is not None else []):
        if where != rel:
            continue
        if text.count(old) != 1:
            raise RuntimeError("mutant %s: its text occurs %d times in %s, not once" % (mutant, text.count(old), rel))
        text = text.replace(old, new)
    return text


def check_copy(texts: dict) -> None:
    """No asm statement and no unknown amdgcn builtin may reach the host compiler."""
    known = standin_builtins()
    for rel, text in texts.items():
        code = _strip_comments(text)
        if re.search(r"\b(asm|__asm__|__asm)\b", code):
            raise RuntimeError("%s: an asm statement survives the rewrites %s" % (rel, sorted(REWRITES)))
        unknown = set(re.findall(r"__builtin_amdgcn_\w+", code)) - known
        if unknown:
            raise RuntimeError("%s uses %s, which the stand-in header does not define" % (rel, sorted(unknown)))
        if "__shared__" in code and re.search(r"extern\s+__shared__", code):
            raise RuntimeError("%s: a dynamic LDS declaration the dynamic_lds rewrite does not know" % rel)


def _want(variant: str, part: str, mutant, texts: dict) -> str:
    h = hashlib.sha256((" ".join(FLAGS[variant] + COMMON) + "\0" + part + "\0" + str(mutant)).encode())
    for path in (MAIN, STANDIN):
        with open(path, "rb") as f:
            h.update(f.read())
    for rel in sorted(texts):
        h.update(rel.encode() + b"\0" + texts[rel].encode())
    return h.hexdigest()


def build(variant: str = "asan", part: str = "perm", mutant=None, verbose: bool = False) -> str:
    """-> path of the executable; rebuilt when a source, the stand-in, the driver, the flags or the mutant changed."""
    texts = {rel: rewritten(rel, mutant) for rel in COPIED}
    check_copy(texts)
    want = _want(variant, part, mutant, texts)
    out_dir = os.path.join(BUILD, "%s_%s" % (variant, part) + ("" if mutant is None else "_" + mutant))
    exe, stamp = os.path.join(out_dir, "hostsim"), os.path.join(out_dir, "hostsim.stamp")
    os.makedirs(out_dir, exist_ok=True)

    def fresh():
        return os.path.exists(exe) and os.path.exists(stamp) and open(stamp).read().strip() == want

    if fresh():
        return exe
    with open(os.path.join(out_dir, "hostsim.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if fresh():
                return exe
            src = os.path.join(out_dir, "src")
            shutil.rmtree(src, ignore_errors=True)
            for rel, text in texts.items():
                os.makedirs(os.path.dirname(os.path.join(src, rel)), exist_ok=True)
                with open(os.path.join(src, rel), "w") as f:
                    f.write(text)
            tmp = exe + ".tmp.%d" % os.getpid()
            cmd = [CLANG] + COMMON + FLAGS[variant] + ["-DHOSTSIM_PART=%d" % PARTS[part], "-I", HOSTSIM, "-I", src, MAIN,
                                                            "-o", tmp]
            if verbose:
                print("[hostsim_lib]", " ".join(cmd), flush=True)
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("hostsim build failed:\n" + r.stderr[-8000:])
            os.replace(tmp, exe)
            with open(stamp + ".tmp", "w") as f:
                f.write(want + "\n")
            os.replace(stamp + ".tmp", stamp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return exe


def build_driver(main_path: str, name: str, variant: str = "asan") -> str:
    """-> path of <directory of main_path>/build/<name>: a stand-alone driver (its own main) over the stand-in header and the
    copied tree, under FLAGS[variant]; rebuilt when the driver, the stand-in, a copied header or the flags change."""
    texts = {rel: rewritten(rel) for rel in COPIED}
    check_copy(texts)
    with open(main_path) as f:
        included = re.findall(r'^#include "((?:include|hades252_amd)/[^"]+)"', f.read(), flags=re.M)
    assert set(included) <= set(texts)
    h = hashlib.sha256(" ".join(FLAGS[variant] + COMMON).encode())
    for path in (main_path, STANDIN):
        with open(path, "rb") as f:
            h.update(f.read())
    for rel in sorted(texts):
        h.update(rel.encode() + b"\0" + texts[rel].encode())
    want = h.hexdigest()
    out_dir = os.path.join(os.path.dirname(main_path), "build")
    os.makedirs(out_dir, exist_ok=True)
    out, stamp = os.path.join(out_dir, name), os.path.join(out_dir, name + ".stamp")

    def fresh():
        return os.path.exists(out) and os.path.exists(stamp) and open(stamp).read().strip() == want

    with open(os.path.join(out_dir, name + ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not fresh():
                src = os.path.join(out_dir, "src")
                for rel, text in texts.items():
                    os.makedirs(os.path.dirname(os.path.join(src, rel)), exist_ok=True)
                    with open(os.path.join(src, rel), "w") as f:
                        f.write(text)
                tmp = out + ".tmp.%d" % os.getpid()
                r = subprocess.run([CLANG] + COMMON + FLAGS[variant] + ["-I", HOSTSIM, "-I", src, main_path, "-o", tmp],
                                   capture_output=True, text=True)
                assert r.returncode == 0, r.stderr[-8000:]
                os.replace(tmp, out)
                with open(stamp + ".tmp", "w") as f:
                    f.write(want + "\n")
                os.replace(stamp + ".tmp", stamp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return out


# every executable the tests use: (variant, part, mutant).  TSan runs the perm, merkle and sponge parts; the mutants live
# in the perm part (k_perm_fast through the shipped launcher, and the unit wrappers).
MUTANT_VARIANT = {"store_off_by_one": "asan", "lds_halved": "asan", "load_barrier_removed": "tsan", "negp_index": "asan",
                  "double_doubled": "asan", "xw_single_buffer": "tsan", "carry_light_shift": "asan",
                  "lanes_word_off_by_one": "asan"}
ALL_BUILDS = [("asan", p, None) for p in PARTS] + [("tsan", p, None) for p in ("perm", "merkle", "sponge")] + \
             [(v, "perm", m) for m, v in MUTANT_VARIANT.items()]
BUILD_JOBS = 6          # compilers side by side in build_all (a fixed number, not the machine's CPU count)


_ALL_BUILT = False


def build_all(builds=None) -> None:
    """Build (or find fresh) every executable in `builds`, BUILD_JOBS at a time: the first hostsim test of a session pays
    for all of them at once instead of each test file for its own."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(BUILD_JOBS) as ex:
        list(ex.map(lambda b: build(*b), builds or ALL_BUILDS))
    if builds is None:
        global _ALL_BUILT
        _ALL_BUILT = True


SAN_ENV = {
    "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=23",
    "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1:exitcode=24",
    "TSAN_OPTIONS": "halt_on_error=1:exitcode=66:report_signal_unsafe=0",
}


class Result:
    def __init__(self, returncode, stdout, stderr, rc, out):
        self.returncode, self.stdout, self.stderr, self.rc, self.out = returncode, stdout, stderr, rc, out


class Script:
    """One run of the executable: buffers in, calls, buffers out.

        s = Script(); s.buf("st", data); s.call("hades252_perm_batch_dev", "st", n, None); s.dump("st")
        r = s.run(timeout=...); r.rc == [("hades252_perm_batch_dev", 0)]; r.out["st"]
    """

    def __init__(self, part: str = "perm", variant: str = "asan", mutant=None):
        self.part, self.variant, self.mutant = part, variant, mutant
        self.lines, self.files, self.dumps = [], {}, []

    def buf(self, name: str, data) -> str:
        self.files[name] = bytes(data)
        self.lines.append(("buf", name))
        return name

    def zero(self, name: str, n_bytes: int) -> str:
        self.lines.append("buf %s zero %d" % (name, n_bytes))
        return name

    def fill(self, name: str, n_bytes: int, value: int) -> str:
        self.lines.append("buf %s fill %d %d" % (name, n_bytes, value))
        return name

    def call(self, func: str, *args) -> None:
        toks = ["null" if a is None else str(int(a)) if not isinstance(a, str) else a for a in args]
        self.lines.append("call %s %s" % (func, " ".join(toks)))

    def dump(self, name: str) -> None:
        self.dumps.append(name)
        self.lines.append(("dump", name))

    def run(self, timeout: float, check: bool = True) -> Result:
        if not _ALL_BUILT:
            build_all()
        exe = build(self.variant, self.part, self.mutant)
        with tempfile.TemporaryDirectory(prefix="hostsim_") as tmp:
            text = []
            for line in self.lines:
                if isinstance(line, tuple) and line[0] == "buf":
                    path = os.path.join(tmp, line[1] + ".in")
                    with open(path, "wb") as f:
                        f.write(self.files[line[1]])
                    text.append("buf %s file %s" % (line[1], path))
                elif isinstance(line, tuple):
                    text.append("dump %s %s" % (line[1], os.path.join(tmp, line[1] + ".out")))
                else:
                    text.append(line)
            r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=timeout,
                               env=dict(os.environ, **SAN_ENV))
            if check:
                assert r.returncode == 0, "hostsim %s exited %d\n%s\n%s" % (self.variant, r.returncode, r.stdout[-2000:],
                                                                            r.stderr[-6000:])
            rc = [(m.group(1), m.group(2)) for m in re.finditer(r"^rc (\w+) (.*)$", r.stdout, flags=re.M)]
            rc = [(f, int(v) if re.fullmatch(r"-?\d+", v) else v) for f, v in rc]
            out = {}
            for name in self.dumps:
                path = os.path.join(tmp, name + ".out")
                if os.path.exists(path):
                    with open(path, "rb") as f:
                        out[name] = f.read()
            return Result(r.returncode, r.stdout, r.stderr, rc, out)


def entry_points(part: str, variant: str = "asan") -> list:
    """The names in the table of one executable."""
    s = Script(part, variant)
    s.lines.append("list")
    return re.findall(r"^entry (\w+)$", s.run(timeout=60).stdout, flags=re.M)        # starts and prints: under a second
