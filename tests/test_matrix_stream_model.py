"""CPU tier: the model of the streaming matrix commitments (tests/matrix_stream_model.py).  Its state is built from the
oracle's permutation and additions alone; here it is tied to the oracle's sponge (tests/matrix_model.py: row_digests) for
every column total that differs in blocks, open block or padding, and shown to be independent of how the columns are split
into groups."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matrix_model as M  # noqa: E402
import matrix_stream_model as MS  # noqa: E402
import oracle_lib  # noqa: E402
from gpu_common import CAP  # noqa: E402

N_ROWS = 7


@pytest.fixture(scope="module")
def matrix(oracle):
    m = oracle.gen_b(16000, N_ROWS * 9).reshape(N_ROWS, 9, 4).copy()
    m[0] = 0                                                           # an all-zero row
    m[1, :] = np.array(oracle_lib.limbs_of(oracle_lib.P - 1), dtype=np.uint64)   # every addition of this row wraps or nearly does
    return m


@pytest.mark.parametrize("pad_mode", [0, 1])
@pytest.mark.parametrize("total", range(1, 10))
def test_finish_equals_the_oracles_sponge(oracle, matrix, total, pad_mode):
    m = matrix[:, :total]
    s = MS.Stream(oracle, N_ROWS).absorb(m)
    before = s.states.copy()
    assert s.digests(pad_mode).tobytes() == M.row_digests(oracle, m, CAP, pad_mode).tobytes()
    assert s.states.tobytes() == before.tobytes() and s.n_cols == total          # finish works on a copy


def test_the_permutation_count_is_the_sponges():
    # hades252_sponge_blocks: 4 columns are one permutation without padding and two with it; 5 are two either way
    assert [MS.permutations(4, 0), MS.permutations(4, 1), MS.permutations(5, 0), MS.permutations(5, 1)] == [1, 2, 2, 2]
    for c in range(1, 40):
        for pad in (0, 1):
            assert MS.permutations(c, pad) == max(1, (c + pad + 3) // 4)


def test_the_state_does_not_depend_on_the_split(oracle, matrix):
    m = matrix[:, :6]
    whole = MS.Stream(oracle, N_ROWS).absorb(m)
    comps = MS.compositions(6)
    assert len(comps) == 32 and len(set(comps)) == 32 and all(sum(c) == 6 for c in comps)
    for groups in comps:
        s = MS.Stream(oracle, N_ROWS)
        for g in MS.split(m, groups):
            s.absorb(g)
        assert s.n_cols == 6 and s.states.tobytes() == whole.states.tobytes(), groups
    # and the state is what the definition says: capacity word and open block after one whole block
    one = MS.Stream(oracle, N_ROWS).absorb(m[:, :3])
    assert (one.states[:, 0] == np.array(oracle_lib.limbs_of(CAP), dtype=np.uint64)).all()      # nothing permuted yet
    assert one.states[2, 1:4].tobytes() == m[2, :3].tobytes() and not one.states[:, 4].any()
    assert one.state_planes().shape == (5, N_ROWS, 4) and one.state_planes()[3, 2].tobytes() == m[2, 2].tobytes()
