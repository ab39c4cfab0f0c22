"""CPU tier: every field routine that tests/units/arith_units.hip wraps -- the per-lane ones, the lane-split ones of
hades_lanes.hpp (units_lane_*, carry_split) and the DPP / permlane moves those are made of -- run from the unchanged headers
in the host build under ASan+UBSan.

The test bodies are those of tests/test_gpu_a13_units.py themselves -- the same operands (the adversarial maximal-limb
operands of tests/test_fast_model.py among them), the same Python models, the same assertions -- called with a stand-in
for the two things they take from the GPU: a `torch` that keeps "device" tensors in host memory, and a `units` library
whose launchers run the host executable.  So the 64-bit column bounds and the 32-bit limb bounds the models assert on
their own restatement become UBSan findings (signed overflow, shifts) on the code that ships; every input buffer is a heap
block of exactly its size.  The output buffers are those test bodies' own (64 guard words behind the data, checked by
their sentinel), so ASan sees the end of a unit's inputs, not of its output."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as HS  # noqa: E402
import test_gpu_a13_units as U  # noqa: E402

_HANDLE0 = 0x7000_0000_0000


class FakeTensor:
    registry = {}

    def __init__(self, arr):
        self.a = np.ascontiguousarray(arr).copy()
        self.handle = _HANDLE0 + 64 * len(FakeTensor.registry)
        FakeTensor.registry[self.handle] = self

    def cuda(self):
        return self

    def cpu(self):
        return self

    def numpy(self):
        return self.a

    def data_ptr(self):
        return self.handle


class _Stream:
    cuda_stream = 0


class _Cuda:
    @staticmethod
    def current_stream():
        return _Stream()

    @staticmethod
    def synchronize():
        pass


class FakeTorch:
    """What tests/test_gpu_a13_units.py uses of torch, on host memory."""
    Tensor = FakeTensor
    int32 = np.int32
    cuda = _Cuda

    @staticmethod
    def full(shape, value, dtype, device):
        return FakeTensor(np.full(shape, value, dtype=dtype))

    @staticmethod
    def from_numpy(a):
        return FakeTensor(a)


class HostUnits:
    """units.NAME(args..., stream): one run of the host executable; every tensor named by an argument goes in as an
    exact-size buffer and comes back as the run left it."""

    def __getattr__(self, name):
        def launch(*args):
            s = HS.Script()
            toks, used = [], []
            for a in args[:-1]:                                    # the last argument is the stream
                if a in FakeTensor.registry:
                    t = FakeTensor.registry[a]
                    bname = "b%d" % len(used)
                    s.buf(bname, t.a.tobytes())
                    used.append((bname, t))
                    toks.append(bname)
                else:
                    toks.append(int(a))
            s.call(name, *toks, None)
            for bname, _ in used:
                s.dump(bname)
            r = s.run(timeout=300)                                 # measured: at most 1.5 s per launch (mont_lin, 2 400 inputs)
            for bname, t in used:
                t.a = np.frombuffer(r.out[bname], dtype=t.a.dtype).reshape(t.a.shape).copy()
            return r.rc[0][1]
        return launch


@pytest.fixture()
def host(monkeypatch):
    monkeypatch.setattr(U, "_record", lambda *a, **k: None)        # the GPU tier's coverage log is not this tier's
    FakeTensor.registry.clear()
    return FakeTorch, HostUnits()


def test_to_from_f29_round_trip(host):
    U.test_to_from_f29_round_trip(*host)


@pytest.mark.parametrize("sqr", [False, True], ids=["mul", "sqr"])
def test_mont_fips_vs_model(host, sqr):
    U.test_mont_fips_vs_model(*host, sqr)


def test_mont_mul_const_and_small_vs_model(host):
    U.test_mont_mul_const_and_small_vs_model(*host)


@pytest.mark.parametrize("steps", [2, 1], ids=["mont_lin", "mont_lin1"])
def test_mont_lin_vs_model(host, steps, monkeypatch):
    U.test_mont_lin_vs_model(*host, steps, monkeypatch)


def test_sbox29_and_add_lazy_vs_model(host):
    U.test_sbox29_and_add_lazy_vs_model(*host)


def test_small_mds_vs_model(host):
    U.test_small_mds_vs_model(*host)


def test_finalize_both_ends_and_every_number_of_subtractions(host):
    U.test_finalize_both_ends_and_every_number_of_subtractions(*host)


def test_finalize32_vs_model(host):
    U.test_finalize32_vs_model(*host)


@pytest.mark.parametrize("ncol", [3, 5])
def test_mds_row_cols_vs_model(host, ncol):
    U.test_mds_row_cols_vs_model(*host, ncol)


def test_fr_is_canonical_word_boundaries(host):
    U.test_fr_is_canonical_word_boundaries(*host)


def test_fr_cond_sub_p_both_tops(host):
    U.test_fr_cond_sub_p_both_tops(*host)


def test_fr_add_and_mul_vs_truth(host):
    U.test_fr_add_and_mul_vs_truth(*host)


# ---- hades_lanes.hpp: the stand-in header emulates the DPP row moves and the permlane swaps (one wave-wide exchange each)
def test_dpp_moves_vs_model(host):
    """The emulation itself, held to the model the MI355X is held to by the GPU tier's run of the same body."""
    U.test_dpp_moves_vs_model(*host)


@pytest.fixture()
def fewer_randoms(monkeypatch):
    """A launch of the lane routines costs two wave barriers per DPP move here: 64 random rows (plus four per mixed wave)
    instead of the GPU tier's 512 to 1 024; every adversarial pattern, and every pair of them, stays."""
    monkeypatch.setattr(U, "N_RANDOM", 256)


def test_lane_mont_mul_and_sbox_vs_model(host, fewer_randoms):
    U.test_lane_mont_mul_and_sbox_vs_model(*host)


def test_lane_lin_vs_model(host, fewer_randoms):
    U.test_lane_lin_vs_model(*host)


def test_lane_mds_row_vs_model(host, fewer_randoms):
    U.test_lane_mds_row_vs_model(*host)


def test_carry_split_vs_model(host, fewer_randoms):
    U.test_carry_split_vs_model(*host)


def test_every_wrapped_routine_is_driven():
    """No launcher of arith_units.hip is out of this tier's reach, and this file has a test for each body of the GPU tier."""
    import units_lib
    reached = set(HS.entry_points("perm"))
    missing = {n for n in list(units_lib._PTRS) + ["units_mds_row_cols", "units_lane_mds_row"] if n not in reached}
    assert missing == set()
    bodies = {n for n in dir(U) if n.startswith("test_")}
    assert bodies <= set(globals()), bodies - set(globals())
