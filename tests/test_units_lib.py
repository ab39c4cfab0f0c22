"""CPU tier guard of the unit library (tests/units/arith_units.hip, driven by tests/test_gpu_a13_units.py): it compiles
with hipcc and the product's flags, and it wraps the SHIPPED routines -- it includes the product's headers and calls the
routines by name, but defines none of them, so the GPU unit tests cannot end up checking a copy."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import units_lib  # noqa: E402

WRAPPED = ["to_f29", "from_f29", "mont_fips", "mont_mul_small", "mont_lin", "mont_lin1", "sbox29", "add_lazy", "small_mds",
           "finalize", "finalize1", "finalize32", "mds_row_cols", "fr_add", "fr_cond_sub_p", "fr_mul", "fr_is_canonical",
           "lane_mont_mul", "lane_lin", "lane_sbox", "lane_mds_row", "carry_split", "row_shr", "row_shl", "row_bcast",
           "wave_bcast_row"]
HEADERS = ["fr32.hpp", "hades_constants.inc", "hades_literal.hpp", "staging.hpp", "hades_fast.hpp", "k_perm_fast.hpp",
           "hades_coop.hpp", "hades_lanes.hpp", "device_tables.hpp", "kernels_perm.hpp"]


def _source():
    with open(units_lib.SRC) as f:
        text = f.read()
    text = re.sub(r"//[^\n]*", "", text)                      # comments may name anything
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_unit_library_wraps_the_shipped_routines_without_defining_them():
    src = _source()
    # the shipped headers, by relative path, in hades252.hip's order
    got = re.findall(r'#include\s+"\.\./\.\./hades252_amd/csrc/([^"]+)"', src)
    assert got == HEADERS
    assert not [f for f in os.listdir(units_lib.UNITS_DIR) if f.endswith((".hpp", ".h", ".inc", ".cuh"))]
    for name in WRAPPED:
        assert re.search(r"\b%s\s*(<[^<>()]*>)?\s*\(" % name, src), "%s is not called" % name
        # a definition: a return type / qualifier, the name, a parameter list and a body
        defn = re.compile(r"(?:__device__|__host__|__forceinline__|inline|static|constexpr|\bFr\b|\bF29\b|\bbool\b|\bvoid\b|"
                          r"u?int(?:32|64)_t|\bauto\b)[^;{}()]*\b%s\s*\([^;{}]*\)\s*(?:const\s*)?\{" % name)
        assert not defn.search(src), "%s is defined in the unit library" % name
        assert not re.search(r"#\s*define\s+%s\b" % name, src)
    assert not re.search(r"\bnamespace\s+hades\s*\{", src), "the unit library must not add to the product's namespace"


def test_unit_library_compiles_with_the_product_flags():
    so = units_lib.build()
    assert os.path.isfile(so) and os.path.getsize(so) > 0
    with open(so + ".stamp") as f:
        assert f.read().strip() == units_lib.source_hash()
