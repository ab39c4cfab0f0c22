// kernels_rowmajor.hpp -- mixed-height matrix commitments from matrices stored ROW by row, and from both layouts in one
// launch: the absorb of several heights and the gather of the opened rows (abi_rowmajor.hpp, host_rowmajor.hpp).  The
// states, the tree, the paths and the verification are those of kernels_matrix_stream.hpp, kernels_merkle.hpp and
// kernels_mmcs.hpp.  Part of the single translation unit hades252.hip (included there after kernels_dmmcs.hpp); not a
// stand-alone header.
#pragma once

// Both kernels, as kernels_dmmcs.hpp: one item per lane, every word is a per-lane load_word / store_word, no LDS, no
// barrier, no scratch (__launch_bounds__(256, 3): at most 168 VGPRs).  A matrix is addressed through two steps, in scalars:
// scalar (r, j) sits at base + (r * row_step + j * col_step) * 32 -- (1, stride) for a column-major matrix, whose lanes then
// read 2 KiB contiguous per column as in kernels_dmmcs.hpp, and (stride, 1) for a row-major one, whose lanes read 32 bytes
// each from rows `stride` scalars apart (k_rm_absorb: the four columns of a block are one 128-byte run per lane) or
// consecutive scalars of one row (k_rm_rows).  The host computes the steps: the kernels know no layout.  Every branch
// depends on kernel arguments and blockIdx only and is uniform over the block, but for the range check of a query's index in
// k_rm_rows.  A lane past its range leaves at once: it reads and writes nothing.

// The parts of one absorb call, by value in the kernel arguments, in the order of the grid: part p owns the blocks
// first_block[p] .. first_block[p + 1] - 1 (the last part: to the end of the grid), lane i of them row i of the part.
//   base      the part's columns, scalar (r, j) at base + (r * row_step + j * col_step) * 32
//   state     the five state planes (kernels_matrix_stream.hpp) of the part's rows, S words apart;  rows: rows of the part
//             (a whole group: rows == S; a row tile of the host form: fewer, and state points at the tile's first row)
//   g         columns of the part;  cur: columns already in the group's open block (its column total mod 4)
struct RmParts {
    const uint8_t *base[HADES252_MMCS_MAX_GROUPS];
    uint8_t *state[HADES252_MMCS_MAX_GROUPS];
    uint64_t S[HADES252_MMCS_MAX_GROUPS];
    uint64_t rows[HADES252_MMCS_MAX_GROUPS];
    uint64_t row_step[HADES252_MMCS_MAX_GROUPS];
    uint64_t col_step[HADES252_MMCS_MAX_GROUPS];
    uint64_t g[HADES252_MMCS_MAX_GROUPS];
    uint32_t first_block[HADES252_MMCS_MAX_GROUPS];
    uint32_t cur[HADES252_MMCS_MAX_GROUPS];
};

// Every part of the table absorbs its columns into its rows' states, in the order of k_planes_absorb: head into the open
// block, body with the next block's four loads in flight across the permutation, tail, the state planes stored at the end.
// `at` is the lane's row (column 0 of the part), `step` the bytes from one column to the next: one body for both layouts.
// Byte equality with the column-major paths holds this copy to theirs (tests/test_rowmajor_cpu_run.py,
// tests/test_gpu_f16_rowmajor.py).
__global__ void __launch_bounds__(kBlock, 3) k_rm_absorb(RmParts parts, uint32_t n_parts) {
    uint32_t p = 0;
    while (p + 1 < n_parts && blockIdx.x >= parts.first_block[p + 1]) p++;
    const size_t S = parts.S[p];
    const size_t row = (size_t)(blockIdx.x - parts.first_block[p]) * kBlock + threadIdx.x;
    if (row >= parts.rows[p]) return;
    uint8_t *__restrict__ state = parts.state[p];
    const uint8_t *__restrict__ at = parts.base[p] + row * parts.row_step[p] * 32;
    const size_t g = parts.g[p], step = parts.col_step[p] * 32;
    const int cur = (int)parts.cur[p];
    Fr st[5];
#pragma unroll
    for (int w = 0; w < 5; w++) st[w] = load_word(state + ((size_t)w * S + row) * 32);
    size_t c = 0;                                                     // columns of the part taken so far
    if (cur != 0) {
        const size_t head = (size_t)(4 - cur) < g ? (size_t)(4 - cur) : g;
#pragma unroll
        for (int k = 1; k < 4; k++)                                   // position k of the open block takes column k - cur
            if (k >= cur && (size_t)(k - cur) < head)
                st[1 + k] = fr_add(st[1 + k], load_word(at + (size_t)(k - cur) * step));
        c = head;
        if ((size_t)cur + head == 4) {
            Fr out[5];
            fast_perm<5>(&d_fast, st, out, 0);
#pragma unroll
            for (int w = 0; w < 5; w++) st[w] = out[w];
        }
    }
    const size_t blocks = (g - c) / 4;
    if (blocks != 0) {
        Fr nxt[4];
#pragma unroll
        for (int k = 0; k < 4; k++) nxt[k] = load_word(at + (c + k) * step);
#pragma unroll 1
        for (size_t t = 0; t < blocks; t++) {
#pragma unroll
            for (int k = 0; k < 4; k++) st[1 + k] = fr_add(st[1 + k], nxt[k]);
            c += 4;
            if (t + 1 < blocks) {                                     // in flight during the permutation
#pragma unroll
                for (int k = 0; k < 4; k++) nxt[k] = load_word(at + (c + k) * step);
            }
            Fr out[5];
            fast_perm<5>(&d_fast, st, out, 0);
#pragma unroll
            for (int w = 0; w < 5; w++) st[w] = out[w];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++)                                       // (after a head that did not close its block c == g)
        if (c + k < g) st[1 + k] = fr_add(st[1 + k], load_word(at + (c + k) * step));
#pragma unroll
    for (int w = 0; w < 5; w++) store_word(state + ((size_t)w * S + row) * 32, st[w]);
}

// The committed matrices of one opening call, tallest first, by value in the kernel arguments.  Group g owns the blocks
// first_block[g] .. first_block[g + 1] - 1 (the last group: to the end of the grid): one lane per (query, column) of it.
//   base    group g's matrix, scalar (r, j) at base + (r * row_step + j * col_step) * 32
//   cols    its columns;  col_off: the columns of the groups before it (its place in a query's output row)
//   div     h_0 / h_g: query index i opens its row i / div
struct RmRowParts {
    const uint8_t *base[HADES252_MMCS_MAX_GROUPS];
    uint64_t row_step[HADES252_MMCS_MAX_GROUPS];
    uint64_t col_step[HADES252_MMCS_MAX_GROUPS];
    uint64_t col_off[HADES252_MMCS_MAX_GROUPS];
    uint32_t cols[HADES252_MMCS_MAX_GROUPS];
    uint32_t div[HADES252_MMCS_MAX_GROUPS];
    uint32_t first_block[HADES252_MMCS_MAX_GROUPS];
};

// rows[q][col_off_g + j] = M_g[indices[q] / div_g][j] for q < n, j < cols_g: the gather of k_dmmcs_rows, its output and its
// split of the grid, through the two steps.  The items of a group run over (query, column) in output order, so for a
// row-major group consecutive lanes read consecutive scalars of the opened row and write consecutive scalars of the output
// row: both sides of the copy are contiguous runs of cols * 32 bytes.  An index >= h_0 stores zeros and loads nothing.
__global__ void __launch_bounds__(kBlock, 3) k_rm_rows(RmRowParts parts, uint32_t n_parts, const uint64_t *__restrict__ indices, size_t n,
                                                       uint64_t h0, size_t row_cols, uint8_t *__restrict__ rows) {
    uint32_t g = 0;
    while (g + 1 < n_parts && blockIdx.x >= parts.first_block[g + 1]) g++;
    const uint32_t cols = parts.cols[g];
    const uint64_t first = (uint64_t)(blockIdx.x - parts.first_block[g]) * kBlock;   // the block's first item of n * cols
    const uint64_t q0 = first / cols;
    const uint32_t at = (uint32_t)(first - q0 * cols) + threadIdx.x;  // < cols + kBlock
    const size_t q = (size_t)q0 + at / cols;
    const uint32_t j = at % cols;
    if (q >= n) return;
    const uint64_t index = indices[q];
    Fr v = zero_word();
    if (index < h0) {
        const uint32_t r = (uint32_t)index / parts.div[g];
        v = load_word(parts.base[g] + ((size_t)r * parts.row_step[g] + (size_t)j * parts.col_step[g]) * 32);
    }
    store_word(rows + (q * row_cols + parts.col_off[g] + j) * 32, v);
}
