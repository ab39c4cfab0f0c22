"""Model of the streaming matrix commitments (hades252_matstream_*): the five-word sponge state of every row after any number
of columns, and the finish rule -- computed through the C oracle's permutation alone (tests/oracle_lib.py: perm_batch) and
additions modulo p on Python integers.  Nothing of the oracle's sponge is used here: tests/test_matrix_stream_model.py ties the
two together.

State of a row after c columns: [capacity, 0, 0, 0, 0], floor(c / 4) blocks of four columns added into words 1..4 and
permuted, the c % 4 columns of the open block added and not permuted.  Finish: under pad_mode 1 Montgomery one joins word
1 + c % 4; a permutation if c % 4 != 0 or pad_mode == 1; the digest is word 1."""
import numpy as np

import oracle_lib
from gpu_common import CAP

ONE_MONT = oracle_lib.R          # the in-memory word of the scalar one


def _ints(a):
    """uint64 [..., 4] -> object array [...] of Python integers."""
    a = np.asarray(a, dtype=np.uint64).astype(object)
    return a[..., 0] + (a[..., 1] << 64) + (a[..., 2] << 128) + (a[..., 3] << 192)


def _limbs(v):
    """object array [...] of Python integers -> uint64 [..., 4]."""
    v = np.asarray(v, dtype=object)
    return np.stack([(v >> (64 * k)) & oracle_lib.M64 for k in range(4)], axis=-1).astype(np.uint64)


def _add_into(states, word, words):
    """states[:, word] += words (mod p), in place; words: uint64 [n_rows, 4]."""
    states[:, word] = _limbs((_ints(states[:, word]) + _ints(words)) % oracle_lib.P)


class Stream:
    """The row states [n_rows, 5, 4] and the column total."""

    def __init__(self, oracle, n_rows, cap=CAP):
        self.oracle, self.n_cols = oracle, 0
        self.states = np.zeros((n_rows, 5, 4), dtype=np.uint64)
        self.states[:, 0] = np.array(oracle_lib.limbs_of(cap), dtype=np.uint64)

    def absorb(self, group):
        """group: row-major uint64 [n_rows, g, 4] -- the next g columns of every row."""
        group = np.asarray(group, dtype=np.uint64)
        assert group.ndim == 3 and group.shape[0] == self.states.shape[0] and group.shape[2] == 4
        for j in range(group.shape[1]):
            _add_into(self.states, 1 + self.n_cols % 4, group[:, j])
            self.n_cols += 1
            if self.n_cols % 4 == 0:
                self.states = self.oracle.perm_batch(self.states.reshape(-1)).reshape(-1, 5, 4)
        return self

    def state_planes(self):
        """The device layout: word w of row r at [w, r] -- uint64 [5, n_rows, 4]."""
        return np.ascontiguousarray(self.states.transpose(1, 0, 2))

    def digests(self, pad_mode=1):
        """uint64 [n_rows, 4]; the state is left as it is."""
        assert self.n_cols > 0 and pad_mode in (0, 1)
        st, open_ = self.states.copy(), self.n_cols % 4
        if pad_mode == 1:
            _add_into(st, 1 + open_, np.tile(np.array(oracle_lib.limbs_of(ONE_MONT), dtype=np.uint64), (st.shape[0], 1)))
        if open_ != 0 or pad_mode == 1:
            st = self.oracle.perm_batch(st.reshape(-1)).reshape(-1, 5, 4)
        return np.ascontiguousarray(st[:, 1])


def permutations(n_cols, pad_mode):
    """Permutations a row has seen once n_cols columns are absorbed and finished: hades252_sponge_blocks(n_cols, pad_mode)."""
    return n_cols // 4 + (1 if n_cols % 4 != 0 or pad_mode == 1 else 0)


def compositions(total):
    """Every way to write `total` as an ordered sum of positive integers: 2^(total - 1) tuples."""
    if total == 0:
        return [()]
    return [(first,) + rest for first in range(1, total + 1) for rest in compositions(total - first)]


def split(matrix, groups):
    """Row-major [n_rows, n_cols, 4] -> the column groups [n_rows, g, 4] in order."""
    assert sum(groups) == matrix.shape[1]
    out, j = [], 0
    for g in groups:
        out.append(np.ascontiguousarray(matrix[:, j:j + g]))
        j += g
    return out
