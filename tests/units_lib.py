"""Build and bind tests/units/libhades252_units.so: the shipped device field routines, one kernel each
(tests/units/arith_units.hip), for tests/test_gpu_a13_units.py.  Test infrastructure only: the product library does not
contain these kernels.

The library is compiled with the product's own hipcc flags (hades252_amd/build.py FLAGS) through the same compile helper
(file lock, temporary file, atomic rename), and is rebuilt when the unit source, any device header of the product or the
flags change."""
import ctypes
import hashlib
import os

from hades252_amd import build as hb

UNITS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "units")
SRC = os.path.join(UNITS_DIR, "arith_units.hip")
SO = os.path.join(UNITS_DIR, "libhades252_units.so")

# launcher -> number of pointer arguments before the count; the ones with a wave-uniform int (MDS row) are listed apart
_PTRS = {"units_to_f29": 2, "units_from_f29": 2, "units_mont_mul": 3, "units_mont_sqr": 2, "units_mont_mul_const": 3,
         "units_mont_mul_small": 3, "units_mont_lin": 3, "units_mont_lin1": 3, "units_sbox29": 2, "units_add_lazy": 3,
         "units_small_mds": 2, "units_finalize": 2, "units_finalize1": 2, "units_finalize32": 2, "units_fr_add": 3,
         "units_fr_cond_sub_p": 3, "units_fr_mul": 3, "units_fr_is_canonical": 2, "units_lane_mont_mul": 3,
         "units_lane_sbox": 2, "units_lane_lin": 3, "units_carry_split": 4, "units_dpp_moves": 3}
_VP, _SZ, _I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def source_hash() -> str:
    h = hashlib.sha256(" ".join(hb.FLAGS).encode())
    with open(SRC, "rb") as f:
        h.update(b"arith_units.hip\0" + f.read())
    for d in hb.DEVICE_DEPS + [os.path.join("..", "..", "include", "hades252.h")]:
        with open(os.path.join(hb.CSRC, d), "rb") as f:
            h.update(d.encode() + b"\0" + f.read())
    return h.hexdigest()


def build(verbose: bool = False) -> str:
    return hb.compile_so(SO, ["arith_units.hip"], source_hash(), UNITS_DIR, verbose=verbose)


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(build())
        for name, k in _PTRS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _I, [_VP] * k + [_SZ, _VP]
        lib.units_mds_row_cols.restype = _I
        lib.units_mds_row_cols.argtypes = [_I, _VP, _I, _VP, _SZ, _VP]
        lib.units_lane_mds_row.restype = _I
        lib.units_lane_mds_row.argtypes = [_VP, _I, _VP, _SZ, _VP]
        _LIB = lib
    return _LIB
