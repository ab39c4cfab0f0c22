"""Row-major matrices for the mixed-height commitments (hades252_rmmcs_absorb_rows, hades252_rmmcs_absorb_ex / _open_ex): the
buffer a row-major caller holds.  There is no hash model here: absorbing a row-major matrix is DEFINED as absorbing the
column-major matrix with the same entries, so the model of it is matrix_stream_model.Stream.absorb / mmcs_model.commit of the
same matrix."""
import numpy as np

import matrix_model as M

LAYOUT_COLS, LAYOUT_ROWS = 0, 1


def rows_of(m, stride=None, gap=M.SENTINEL):
    """Row-major [n_rows, n_cols, 4] -> the row-major buffer [n_rows, stride, 4]; scalars n_cols .. stride - 1 of every row
    (the gap between two rows) hold `gap` in every limb.  The counterpart of matrix_model.planes_of."""
    m = np.ascontiguousarray(m, dtype=np.uint64)
    n_rows, n_cols = m.shape[0], m.shape[1]
    stride = n_cols if stride is None else stride
    assert stride >= n_cols
    rows = np.full((n_rows, stride, 4), gap, dtype=np.uint64)
    rows[:, :n_cols] = m
    return rows


def exact(buf, n_rows, n_cols, layout):
    """The bytes of a buffer of rows_of (LAYOUT_ROWS: [n_rows, stride, 4]) or matrix_model.planes_of (LAYOUT_COLS: [n_cols,
    stride, 4]) up to and including its last scalar: the last row ends with its last column, the last plane with its last
    row."""
    stride = buf.shape[1]
    last = (n_rows - 1) * stride + n_cols if layout == LAYOUT_ROWS else (n_cols - 1) * stride + n_rows
    return buf.reshape(-1)[:last * 4].tobytes()
