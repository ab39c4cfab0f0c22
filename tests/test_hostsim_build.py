"""CPU tier: the host simulation build itself (tests/hostsim_lib.py).  The sources it compiles are the tree's, changed by
nothing but the allow-list of rewrites; a new asm statement or amdgcn builtin breaks the build; the host sources define
none of the routines they run; every device-pointer entry point and every size-dispatched form is either exercised by a
tests/test_hostsim_*.py case or listed, with the one admissible reason, in tests/hostsim/not_emulated.json (empty since
the stand-in header emulates the DPP row moves and the permlane swaps)."""
import glob
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as HS  # noqa: E402
from gpu_common import FORM_SIZES  # noqa: E402
from hades252_amd import build as hb  # noqa: E402

REASON = "needs a builtin the stand-in header does not emulate"


def test_copy_differs_from_the_tree_by_the_allow_list_only():
    changed = 0
    for rel in HS.COPIED:
        with open(os.path.join(ROOT, rel)) as f:
            tree = f.read().split("\n")
        copy = HS.rewritten(rel).split("\n")
        assert len(tree) == len(copy), rel
        for a, b in zip(tree, copy):
            if a == b:
                continue
            changed += 1
            images = [pat.sub(repl, a) for pat, repl in HS.REWRITES.values() if pat.search(a)]
            assert images, (rel, a)
            text = a
            for pat, repl in HS.REWRITES.values():
                text = pat.sub(repl, text)
            assert b == text, (rel, a, b)
    assert changed > 20                                    # the fences and the dynamic LDS declarations are there to be rewritten


def test_every_compiled_device_source_is_a_source_of_the_product():
    """Every file of hades252_amd/build.py's dependency list that holds device code or launch policy is in the copy."""
    deps = hb.DEVICE_DEPS + hb.LAUNCH_POLICY_DEPS + hb.UNRECORDED_KERNEL_DEPS + ["abi_util.hpp"]
    assert {os.path.join("hades252_amd", "csrc", d) for d in deps} <= set(HS.COPIED)
    with open(HS.MAIN) as f:
        main = f.read()
    for d in deps:
        assert '#include "hades252_amd/csrc/%s"' % d in main, d
    for d in hb.HOST_DEPS:
        if d.startswith("host_") and d != "host_fault.hpp":
            assert d not in main, "host plumbing in the host simulation: %s" % d


def test_build_refuses_a_new_asm_statement_and_an_unknown_builtin():
    rel = os.path.join("hades252_amd", "csrc", "hades_fast.hpp")
    text = HS.rewritten(rel)
    HS.check_copy({rel: text})
    with pytest.raises(RuntimeError, match="asm statement survives"):
        HS.check_copy({rel: text + '\ninline void f(int &x) { asm volatile("v_nop" : "+v"(x)); }\n'})
    with pytest.raises(RuntimeError, match="asm statement survives"):
        HS.check_copy({rel: text + '\ninline void f() { __asm__("s_nop 0"); }\n'})
    with pytest.raises(RuntimeError, match="does not define"):
        HS.check_copy({rel: text + "\ninline int f(int x) { return __builtin_amdgcn_mov_dpp8(x, 0); }\n"})
    with pytest.raises(RuntimeError, match="dynamic LDS"):
        HS.check_copy({rel: text + "\ninline void f() { extern __shared__ float other[]; }\n"})
    assert "__builtin_amdgcn_wave_barrier" in HS.standin_builtins()


def test_mutants_apply_to_exactly_one_place():
    for name in HS.MUTANTS:
        for rel, old, new in HS.mutant_edits(name):      # (a mutant may be several edits that belong together)
            assert HS.rewritten(rel).count(old) == 1 and old != new, name
            assert HS.rewritten(rel, name) != HS.rewritten(rel), name
            assert HS.rewritten(rel, name).count(new) == 1, name


def _code(path):
    with open(path) as f:
        return HS._strip_comments(f.read())


def test_host_sources_define_none_of_the_routines_they_run():
    """In the spirit of tests/test_units_lib.py: no function of the device headers, no kernel and no entry point is defined
    (or even named, outside the driver's table) in tests/hostsim."""
    names = set()
    for rel in HS.COPIED:
        if rel.endswith("hades252.h"):
            continue
        code = _code(os.path.join(ROOT, rel))
        names |= set(re.findall(r"(?:__device__|__global__)[^;{}()]*?\b(\w+)\s*\(", code))
        names |= set(re.findall(r"__global__[^;{]*?\b([ku]_\w+)\s*\(", code))
        names |= set(re.findall(r"^(?:static )?(?:inline )?(?:int|size_t|void|bool|Fr|unsigned)\s+(\w+)\s*\(", code, flags=re.M))
    names -= {"defined", "aligned", "__launch_bounds__", "__attribute__", "if", "for", "while", "return", "sizeof", "main", "operator"}
    assert {"fast_perm", "mont_fips", "k_perm_fast", "fr_mul", "wave_load_scalars", "hades252_perm_batch_dev_ex",
            "launch_perm_fast", "merkle_run"} <= names
    main = re.sub(r"REG\(\w+\);|#include [^\n]*", "", _code(HS.MAIN))
    assert "__global__" not in main and "__device__" not in main          # no kernel and no device routine, whatever its name
    # The form launchers (namespace forms) launch shipped kernels at sizes the dispatch would not give them: there, and only
    # there, the driver names kernels -- as launch targets -- and the three host helpers their call sites pass arguments
    # through.  Outside that block the rule is the old one.
    head, rest = main.split("namespace forms {")
    block, tail = rest.split("using namespace forms;")
    in_block = {n for n in names if re.search(r"\b%s\b" % re.escape(n), block)}
    assert in_block and in_block <= {n for n in names if n.startswith("k_")} | {"fr_from_u64", "fr_mont_of_u64", "safe_plan"}
    for k in (n for n in in_block if n.startswith("k_")):                  # every mention of a kernel is a launch target
        for m in re.finditer(r"\b%s\b" % k, block):
            before = block[:m.start()]
            assert before.rfind("FORM_LAUNCH(") > before.rfind(";"), k
    main = head + tail
    standin = _code(HS.STANDIN)
    for text, where in ((main, "hostsim_main.cpp"), (standin, "hip_runtime.h")):
        used = {n for n in names if re.search(r"\b%s\b" % re.escape(n), text)}
        assert not used, (where, sorted(used))


def _test_sources():
    out = ""
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_hostsim_*.py"))):
        if not path.endswith("test_hostsim_build.py"):
            with open(path) as f:
                out += f.read()
    return out


def test_every_entry_point_and_form_is_exercised_or_excluded_for_dpp():
    with open(os.path.join(ROOT, "include", "hades252.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    exports = sorted(set(re.findall(r"\b(hades252_\w+_dev(?:_ex)?)\s*\(", header)))
    assert len(exports) > 50
    with open(os.path.join(HS.HOSTSIM, "not_emulated.json")) as f:
        excluded = json.load(f)
    assert all(e["reason"] == REASON for e in excluded)
    skip = {e["name"] for e in excluded}
    assert excluded == []                                  # nothing is out of reach today; the mechanism stays for a future builtin
    # an excluded ENTRY POINT (not a form) must say why no call of it can reach an emulated form
    for e in excluded:
        if not e["name"].startswith("form:"):
            assert e.get("why"), e["name"]
    # hades252_merkle_empty_digests_dev launches nothing but launch_merkle_lanes with one parent (its test relies on it)
    with open(os.path.join(hb.CSRC, "abi_merkle.hpp")) as f:
        body = f.read().split("int hades252_merkle_empty_digests_dev(")[1].split("\nint hades252_")[0]
    assert set(re.findall(r"\b(launch_\w+|hipLaunchKernelGGL\(\w+)", body)) == {"launch_merkle_lanes", "hipLaunchKernelGGL(k_store_fr"}
    # "exercised" is textual: the quoted name stands in a tests/test_hostsim_*.py file (every such string there is the
    # function of a Script.call or the expected name of its printed status)
    tests = _test_sources()
    called = set(re.findall(r'"(hades252_\w+)"', tests))
    in_table = set(sum((HS.entry_points(p) for p in HS.PARTS), []))
    for name in exports:
        assert name in in_table, "%s is not in the host build's table" % name
        assert (name in called) != (name in skip), "%s: %s" % (
            name, "exercised AND excluded" if name in called else "neither exercised by a hostsim test nor excluded")
    for form in FORM_SIZES:
        used = re.search(r'(FORM_SIZES|LEVEL_SIZES)\["%s"\]' % form, tests) is not None
        assert used != ("form:" + form in skip), form
    assert skip <= set(exports) | {"form:" + f for f in FORM_SIZES}
