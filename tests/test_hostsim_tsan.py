"""CPU tier: the kernels that exchange data through LDS, run from the unchanged sources in the host build under
ThreadSanitizer.  Every lane is an OS thread and every `__syncthreads` / wave barrier the only ordering there is, so a
missing barrier between an LDS write and another lane's read is a data-race report whatever the schedule happened to be
(tests/test_hostsim_mutants.py removes one to prove it).  Outputs are still compared with the oracle."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as HS  # noqa: E402
import oracle_lib  # noqa: E402
import cipher_model as CM  # noqa: E402
from oracle_lib import limbs_of  # noqa: E402
from gpu_common import CAP, TAG, edge_scalars, FORM_SIZES  # noqa: E402

FAST, COOP = 2, 3


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def u64(b):
    return np.frombuffer(b, dtype=np.uint64)


def limbs(v):
    return np.array(limbs_of(v), dtype=np.uint64).tobytes()


def test_perm_fast_coop_and_the_traces(oracle):
    """k_perm_fast (staging.hpp, block barriers), k_perm_coop (one barrier per round, ping-pong exchange), the true trace
    and the scaled trace (slab_flush_wave: wave barriers only)."""
    n = 300
    inp = edge_scalars(5 * n, 600)
    s = HS.Script("perm", "tsan")
    for name, k in (("fast", FAST), ("coop", COOP)):
        s.buf(name, inp.tobytes())
        s.call("hades252_perm_batch_dev_ex", name, n, None, k)
        s.dump(name)
    nt = 70
    s.buf("st", inp[:20 * nt].tobytes())
    s.fill("tr", 67 * 160 * nt, 0xFF)
    s.fill("trs", 67 * 160 * nt, 0xFF)
    s.call("hades252_perm_trace_dev", "st", "tr", nt, None)
    s.call("hades252_perm_trace_scaled_dev", "st", "trs", nt, None)
    s.dump("tr")
    r = s.run(timeout=900)                               # measured: 6 s
    assert [rc for _, rc in r.rc] == [0, 0, 0, 0]
    exp = oracle.perm_batch(inp)
    assert (u64(r.out["fast"]) == exp).all() and (u64(r.out["coop"]) == exp).all()
    trace = u64(r.out["tr"]).reshape(67, nt, 20)
    assert (trace[66] == exp[:20 * nt].reshape(nt, 20)).all()
    assert (trace[0, 0] == oracle.perm_trace(inp[:20])[1][0].reshape(-1)).all()


def test_fused_merkle_coop_launch(oracle, monkeypatch):
    """The two-level k_merkle_coop launch of merkle_run (arity 2, 2^15 leaves): level 1 stays in LDS for level 2."""
    monkeypatch.setenv("HOSTSIM_DPP_MAX_BLOCKS", "0")
    leaves = edge_scalars(1 << 15, 601)
    levels = oracle.merkle_tree(leaves, 2, TAG[2], 1)
    tree_bytes = 8 * sum(l.size for l in levels)
    s = HS.Script("merkle", "tsan")
    s.buf("leaves", leaves.tobytes())
    s.buf("tag", limbs(TAG[2]))
    s.fill("tree", tree_bytes, 0xFF)
    s.call("hades252_merkle_build_dev", "leaves", 1 << 15, 2, "tag", 1, "tree", None)
    s.dump("tree")
    r = s.run(timeout=2400)                              # measured: 52 s
    assert r.rc == [("hades252_merkle_build_dev", 0)]
    two = np.concatenate(levels[:2])
    assert (u64(r.out["tree"])[:two.size] == two).all()


def test_sponge_sort_per_lane_sponge_and_cipher(oracle):
    """The counting sort (LDS histograms, block scan), then k_sponge on the sorted order; one per-lane cipher launch."""
    n = FORM_SIZES["fast"][0]
    n_pool = 2000
    pool = edge_scalars(n_pool, 602)
    rng = np.random.default_rng(603)
    lens = rng.integers(0, 9, size=n, dtype=np.uint64)
    offs = rng.integers(0, n_pool - 8, size=n, dtype=np.uint64)
    s = HS.Script("sponge", "tsan")
    s.buf("pool", pool.tobytes())
    s.buf("offs", offs.tobytes())
    s.buf("lens", lens.tobytes())
    s.buf("cap", limbs(CAP))
    s.fill("dig", 32 * n, 0xFF)
    s.zero("bad", 4)
    s.fill("scratch", 8 * n + 16384, 0xFF)
    s.call("hades252_sponge_hash_var_ex_dev", "pool", n_pool, "offs", "lens", n, "cap", 1, "dig", "bad", "scratch",
           8 * n + 16384, None)
    s.dump("dig")
    nc, m = 1025, 2
    msgs, keys, nonces = edge_scalars(nc * m, 604), edge_scalars(2 * nc, 605), edge_scalars(nc, 606)
    s.buf("msgs", msgs.tobytes())
    s.buf("keys", keys.tobytes())
    s.buf("nonces", nonces.tobytes())
    s.buf("dom", limbs(CM.DOMAIN_MONT))
    s.fill("c", 32 * nc * (m + 1), 0xFF)
    s.call("hades252_cipher_encrypt_dev", "msgs", "keys", "nonces", nc, m, "dom", "c", None)
    s.dump("c")
    r = s.run(timeout=1800)                              # measured: 20 s
    assert [rc for _, rc in r.rc] == [0, 0]
    assert (u64(r.out["dig"]) == oracle.sponge_var(pool, offs, lens, CAP, 1)).all()
    exp_c = CM.encrypt_batch(msgs.reshape(nc, m, 4), keys.reshape(nc, 2, 4), nonces.reshape(nc, 4), m, oracle.perm_batch)
    assert (u64(r.out["c"]).reshape(exp_c.shape) == exp_c).all()


# ---- the DPP forms of hades_lanes.hpp: where waves meet through LDS -----------------------------------------------------
# The helped form's main waves and helper wave exchange word 3 through LanesLds::xw with one block barrier per full round;
# every DPP move is a wave-wide exchange in the emulator, so what TSan orders by is the barriers the SOURCE has
# (tests/test_hostsim_mutants.py puts both sides on one buffer to prove the detector live).
LANES, ROWS = 4, 5


def test_perm_lanes_helped_and_rows(oracle):
    """k_perm_lanes<true>, four states: a full block, then a block with one state wave, two idle waves and the helper;
    k_perm_rows, five states (rows never meet: the wave's own LDS round trips only)."""
    assert FORM_SIZES["lanes_helped"][0] <= 4 < FORM_SIZES["lanes"][0]
    s = HS.Script("perm", "tsan")
    inp = {}
    for name, n, k in (("lanes", 4, LANES), ("rows", 5, ROWS)):
        inp[name] = edge_scalars(5 * n, 610 + n)
        s.buf(name, inp[name].tobytes())
        s.call("hades252_perm_batch_dev_ex", name, n, None, k)
        s.dump(name)
    r = s.run(timeout=900)                               # measured: 9 s + 7 s
    assert [rc for _, rc in r.rc] == [0, 0]
    for name in inp:
        assert (u64(r.out[name]) == oracle.perm_batch(inp[name])).all(), name


def test_sponge_and_duplex_sponge_lanes_helped(oracle):
    """k_sponge_lanes<true> on four ragged messages (the waves of a block run to the block's maximum) and
    k_safe_lanes<true> on four sponges, one-shot: several permutations per launch, so the buffers of one permutation's last
    rounds meet the next one's first."""
    import safe_model as SM
    import hades_spec as S
    n = 4
    lens = [5, 2, 0, 3]
    pool = edge_scalars(sum(lens), 620)
    offs, la = np.cumsum([0] + lens[:-1]).astype(np.uint64), np.array(lens, dtype=np.uint64)
    s = HS.Script("sponge", "tsan")
    s.buf("pool", pool.tobytes())
    s.buf("offs", offs.tobytes())
    s.buf("lens", la.tobytes())
    s.buf("cap", limbs(CAP))
    s.fill("dig", 32 * n, 0xFF)
    s.zero("bad", 4)
    s.call("hades252_sponge_hash_var_dev", "pool", sum(lens), "offs", "lens", n, "cap", 1, "dig", "bad", None)
    s.dump("dig")
    pat = [SM.A(5), SM.Q(1)]
    tag = S.to_mont(0x1234)
    inp = edge_scalars(n * 5, 621).reshape(n, 5, 4)
    s.buf("tag", limbs(tag))
    s.buf("in", inp.tobytes())
    s.buf("calls", np.array(SM.encode(pat), dtype=np.uint32).tobytes())
    s.fill("out", 32 * n, 0xFF)
    s.call("hades252_safe_hash_dev", "in", n, "calls", len(pat), "tag", "out", None)
    s.dump("out")
    r = s.run(timeout=1200)                              # measured: 40 s
    assert [rc for _, rc in r.rc] == [0, 0]
    assert (u64(r.out["dig"]) == oracle.sponge_var(pool, offs, la, CAP, 1)).all()
    want = SM.run_batch(pat, inp, tag, oracle.perm_batch)
    assert (u64(r.out["out"]).reshape(want.shape) == want).all()
