"""GPU tier, row f11 (beyond SURVEY section 8): the permutation run backwards (hades252_perm_inverse_batch / _rounds) and batched
fifth roots (hades252_fifth_root_batch) against the big-integer model (tests/perm_inverse_model.py), the C oracle's forward
permutation and the library's own forward calls.  Exact, byte for byte, everywhere; at most 2^14 + 3 states per case."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perm_inverse_model as M  # noqa: E402
import round_inverse as RI  # noqa: E402
from gpu_common import EDGE_VALUES, placed_batches, to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

S, P = M.S, M.P
N_BIG = (1 << 14) + 3
SENTINEL = 0xABCDEF0123456789
GUARD = 3                                  # sentinel states (or scalars) on each side of the batch


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "perm_inverse_kat.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pairs(oracle):
    """(x, y): N_BIG generator-B states and their permutations by the C oracle, uint64 [N_BIG, 5, 4]; never written."""
    x = oracle.gen_b(1100, N_BIG * 5).reshape(N_BIG, 5, 4)
    y = oracle.perm_batch(x).reshape(N_BIG, 5, 4)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _ints(hexes):
    return [int(v, 16) for v in hexes]


def _guarded(lib_call, data, *args):
    """`data` (uint64 [n, ...]) in the middle of a larger host array whose rows before and after hold a sentinel: the call
    works in place on the middle; -> the middle, after checking that the sentinel rows still stand."""
    n = data.shape[0]
    big = np.full((n + 2 * GUARD,) + data.shape[1:], SENTINEL, dtype=np.uint64)
    big[GUARD:GUARD + n] = data
    row_bytes = big[0].nbytes
    assert lib_call(ctypes.c_void_p(big.ctypes.data + GUARD * row_bytes), n, *args) == 0
    assert (big[:GUARD] == SENTINEL).all() and (big[GUARD + n:] == SENTINEL).all(), "a row outside the batch was written"
    return big[GUARD:GUARD + n]


# ---- 1. known answers --------------------------------------------------------------------------------------------------
def test_kats_one_call_each_and_all_in_one_call(hades_lib, H, golden):
    assert int(golden["D"], 16) == M.D
    ys = [_ints(c["y"]) for c in golden["perm_inverse"]]
    xs = [_ints(c["x"]) for c in golden["perm_inverse"]]
    for y, x in zip(ys, xs):
        assert H.perm_inverse(M.states_of([y])).tobytes() == M.states_of([x]).tobytes()
    assert H.perm_inverse(M.states_of(ys)).tobytes() == M.states_of(xs).tobytes()
    assert len(golden["inverse_rounds"]) == len(M.ROUND_RANGES)
    for c in golden["inverse_rounds"]:
        got = H.perm_inverse_rounds(M.states_of([_ints(c["in"])]), c["round_hi"], c["round_lo"])
        assert got.tobytes() == M.states_of([_ints(c["out"])]).tobytes(), (c["round_hi"], c["round_lo"])
    vals = [int(c["x"], 16) for c in golden["fifth_root"]]
    roots = [int(c["root"], 16) for c in golden["fifth_root"]]
    words = [int(c["word"], 16) for c in golden["fifth_root_word"]]
    root_words = [int(c["root_word"], 16) for c in golden["fifth_root_word"]]
    for a, b in list(zip(M.scalars_of(vals), M.scalars_of(roots))) + list(zip(M.words_of(words), M.words_of(root_words))):
        assert H.fifth_root(a.reshape(1, 4)).tobytes() == b.tobytes()
    every = np.concatenate([M.scalars_of(vals), M.words_of(words)])
    assert H.fifth_root(every).tobytes() == np.concatenate([M.scalars_of(roots), M.words_of(root_words)]).tobytes()


# ---- 2. sizes and neighbours -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_and_neighbours(hades_lib, pairs, n):
    x, y = pairs
    got = _guarded(hades_lib.hades252_perm_inverse_batch, y[:n])
    assert got.tobytes() == x[:n].tobytes()
    got = _guarded(hades_lib.hades252_perm_inverse_rounds, y[:n], 67, 0)
    assert got.tobytes() == x[:n].tobytes()


# ---- 3. round trip with the library's own forward call ------------------------------------------------------------------
def test_round_trip_with_the_forward_call(hades_lib, H, pairs):
    x, _ = pairs
    fwd = x.copy()
    H.ScalarStrategy().perm(fwd)
    assert H.perm_inverse(fwd).tobytes() == x.tobytes()
    back = H.perm_inverse(x)
    assert back.tobytes() != x.tobytes()
    H.ScalarStrategy().perm(back)
    assert back.tobytes() == x.tobytes()


# ---- 4. edge values inside the rounds ------------------------------------------------------------------------------------
def test_edge_values_inside_the_rounds(hades_lib, H, pairs):
    """Every entry of round_inverse.edge_catalogue(): perm(entry input) in, the entry's input out -- the roots and the exits
    pass through 0, 1, -1 and the in-memory edge words at every catalogued round.  n = 257 places the entries at lanes 0,
    63, 64, 255 and n - 1 of batches otherwise filled with generator-B outputs."""
    cat = RI.edge_catalogue()
    inputs = [list(inp) for inp, _ in cat]
    xs = M.states_of(inputs).reshape(-1, 20)
    ys = M.states_of([S.perm(inp) for inp in inputs]).reshape(-1, 20)
    n = 257
    x_fill, y_fill = pairs[0][:n].reshape(n, 20), pairs[1][:n].reshape(n, 20)
    seen = 0
    for batch, lanes, idx in placed_batches(ys, n, y_fill):
        assert set(lanes) <= {0, 63, 64, 255, n - 1}
        got = H.perm_inverse(np.ascontiguousarray(batch).reshape(n, 5, 4)).reshape(n, 20)
        want = x_fill.copy()
        want[lanes] = xs[idx]
        bad = [str(cat[i][1]) for lane, i in zip(lanes, idx) if got[lane].tobytes() != want[lane].tobytes()]
        assert not bad, bad
        assert got.tobytes() == want.tobytes()
        seen += len(idx)
    assert seen == len(cat) > 100


# ---- 5. round ranges -----------------------------------------------------------------------------------------------------
def test_round_ranges(hades_lib, H, pairs):
    n = 65
    inputs = M.state_values(pairs[0][100:100 + n])
    inputs[0], inputs[63], inputs[64] = [0] * 5, [1] * 5, [P - 1] * 5
    traces = []
    for inp in inputs:
        tr = []
        S.perm(inp, tr)
        traces.append(tr)
    for hi, lo in M.ROUND_RANGES:
        states_in = M.states_of([tr[hi - 1] for tr in traces])
        want = M.states_of([tr[lo - 1] if lo else inp for tr, inp in zip(traces, inputs)])
        got = H.perm_inverse_rounds(states_in, hi, lo)
        assert got.tobytes() == want.tobytes(), (hi, lo)
    assert H.perm_inverse_rounds(states_in, 40, 40).tobytes() == states_in.tobytes()


# ---- 6. fifth roots ------------------------------------------------------------------------------------------------------
def _check_roots(torch, hades_lib, H, scalars):
    """Roots through the C entry point (guarded) and the wrapper; root^5 == x in Python; the library's own forward S-box gives
    the inputs back."""
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    roots = _guarded(hades_lib.hades252_fifth_root_batch, scalars)
    assert H.fifth_root(scalars).tobytes() == roots.tobytes()
    assert all(M.mont_of(row) < P for row in roots)                # fully reduced
    assert [pow(r, 5, P) for r in M.values_of(roots)] == M.values_of(scalars)
    dev = to_dev(torch, roots)
    H.ScalarStrategy().quintic_s_box(dev)
    assert to_host(dev).tobytes() == scalars.tobytes()
    return roots


def test_fifth_roots_of_edge_values(torch_cuda, hades_lib, H):
    """The values 0, 1, 2, -1 and the in-memory edge words (gpu_common.EDGE_VALUES: word boundaries, R, p - R, 2^255 mod p, ..)."""
    words = sorted({v % P for v in EDGE_VALUES} | {S.to_mont(v) for v in (0, 1, 2, P - 1)} | {1, P - 1})
    roots = _check_roots(torch_cuda, hades_lib, H, M.words_of(words))
    by_word = dict(zip(words, (M.mont_of(r) for r in roots)))
    assert by_word[0] == 0 and by_word[S.to_mont(1)] == S.to_mont(1) and by_word[S.to_mont(P - 1)] == S.to_mont(P - 1)


@pytest.mark.parametrize("n", [1, 65, 1025, 4096])
def test_fifth_roots(torch_cuda, hades_lib, H, oracle, n):
    _check_roots(torch_cuda, hades_lib, H, oracle.gen_b(7000, 4096 * 4).reshape(-1, 4)[:n])


# ---- 7. chunking ---------------------------------------------------------------------------------------------------------
_CHUNK_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from hades252_amd import build, strategy as H
build.build(verbose=False)
assert os.environ["HADES252_HOST_CHUNK_BYTES"] == "48000"
src, dst = sys.argv[1], sys.argv[2]
y = np.fromfile(src, dtype=np.uint64)
states, scalars = y[:1000 * 20].reshape(1000, 5, 4), y[1000 * 20:].reshape(-1, 4)
out = np.concatenate([H.perm_inverse(np.ascontiguousarray(states)).reshape(-1), H.fifth_root(np.ascontiguousarray(scalars)).reshape(-1)])
out.tofile(dst)
print("CHUNKED", states.shape[0], scalars.shape[0])
"""


def test_chunked_call_gives_the_single_chunk_bytes(torch_cuda, hades_lib, H, pairs, tmp_path):
    """HADES252_HOST_CHUNK_BYTES = 48000 (read once by the library, hence a child process): 300 states per chunk, so 1000
    states are four chunks with a ragged last one -- the two buffers are each used twice; 4096 scalars are three chunks."""
    x, y = pairs
    states, scalars = np.ascontiguousarray(y[:1000]), np.ascontiguousarray(x.reshape(-1, 4)[:4096])
    single = np.concatenate([H.perm_inverse(states).reshape(-1), H.fifth_root(scalars).reshape(-1)])
    assert single[:1000 * 20].tobytes() == x[:1000].tobytes()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([states.reshape(-1), scalars.reshape(-1)]).tofile(src)
    env = dict(os.environ, HADES252_HOST_CHUNK_BYTES="48000")
    r = subprocess.run([sys.executable, "-c", _CHUNK_CHILD, str(src), str(dst)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "CHUNKED 1000 4096" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    assert np.fromfile(dst, dtype=np.uint64).tobytes() == single.tobytes()
