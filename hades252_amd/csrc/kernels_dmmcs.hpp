// kernels_dmmcs.hpp -- device-resident mixed-height matrix commitments: the absorb of several heights in one launch and the
// gather of the opened rows (abi_dmmcs.hpp).  The tree, the paths and the verification are kernels_merkle.hpp's and
// kernels_mmcs.hpp's.  Part of the single translation unit hades252.hip (included there after kernels_mmcs.hpp); not a
// stand-alone header.
#pragma once

// Both kernels, as kernels_matrix_stream.hpp and kernels_mmcs.hpp: one item per lane, consecutive lanes own consecutive
// items, every word is a per-lane load_word / store_word (32 contiguous bytes per lane, 2 KiB contiguous over the wave).
// No LDS, no barrier, no scratch: registers alone decide the residency (__launch_bounds__(256, 3): at most 168 VGPRs).
// Every branch depends on kernel arguments and blockIdx only and is uniform over the block, but for the range check of a
// query's index in k_dmmcs_rows; the state words are indexed by unrolled constants.  A lane past its range leaves at once: it
// reads and writes nothing.

// The parts of one absorb call, by value in the kernel arguments, in the order of the grid: part p owns the blocks
// first_block[p] .. first_block[p + 1] - 1 (the last part: to the end of the grid), lane i of them row i of its group.
//   planes  the part's columns, scalar (r, j) at planes + (j * stride + r) * 32
//   state   the group's five state planes (kernels_matrix_stream.hpp), S rows each
//   g       columns of the part;  cur: columns already in the group's open block (its column total mod 4)
struct DmmcsParts {
    const uint8_t *planes[HADES252_MMCS_MAX_GROUPS];
    uint8_t *state[HADES252_MMCS_MAX_GROUPS];
    uint64_t S[HADES252_MMCS_MAX_GROUPS];
    uint64_t stride[HADES252_MMCS_MAX_GROUPS];
    uint64_t g[HADES252_MMCS_MAX_GROUPS];
    uint32_t first_block[HADES252_MMCS_MAX_GROUPS];
    uint32_t cur[HADES252_MMCS_MAX_GROUPS];
};

// Every part of the table absorbs its columns into its group's row states: for its row each lane does exactly what
// k_planes_absorb does (head, body with the next block's four loads in flight across the permutation, tail), so the short
// groups' chains of permutations run beside the tall group's instead of after it.  The block finds its part from blockIdx.x
// alone, a scalar search over at most 32 entries.  The body below is a second copy of k_planes_absorb's: byte equality with
// the host path holds the two together (tests/test_dmmcs_cpu_run.py, tests/test_gpu_f15_dmmcs.py).
__global__ void __launch_bounds__(kBlock, 3) k_dmmcs_absorb(DmmcsParts parts, uint32_t n_parts) {
    uint32_t p = 0;
    while (p + 1 < n_parts && blockIdx.x >= parts.first_block[p + 1]) p++;
    const size_t S = parts.S[p];
    const size_t row = (size_t)(blockIdx.x - parts.first_block[p]) * kBlock + threadIdx.x;
    if (row >= S) return;
    uint8_t *__restrict__ state = parts.state[p];
    const uint8_t *__restrict__ planes = parts.planes[p];
    const size_t g = parts.g[p], stride = parts.stride[p];
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
                st[1 + k] = fr_add(st[1 + k], load_word(planes + ((size_t)(k - cur) * stride + row) * 32));
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
        for (int k = 0; k < 4; k++) nxt[k] = load_word(planes + ((c + k) * stride + row) * 32);
#pragma unroll 1
        for (size_t t = 0; t < blocks; t++) {
#pragma unroll
            for (int k = 0; k < 4; k++) st[1 + k] = fr_add(st[1 + k], nxt[k]);
            c += 4;
            if (t + 1 < blocks) {                                     // in flight during the permutation
#pragma unroll
                for (int k = 0; k < 4; k++) nxt[k] = load_word(planes + ((c + k) * stride + row) * 32);
            }
            Fr out[5];
            fast_perm<5>(&d_fast, st, out, 0);
#pragma unroll
            for (int w = 0; w < 5; w++) st[w] = out[w];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++)                                       // (after a head that did not close its block c == g)
        if (c + k < g) st[1 + k] = fr_add(st[1 + k], load_word(planes + ((c + k) * stride + row) * 32));
#pragma unroll
    for (int w = 0; w < 5; w++) store_word(state + ((size_t)w * S + row) * 32, st[w]);
}

// The committed matrices of one opening call, tallest first, by value in the kernel arguments.  Group g owns the blocks
// first_block[g] .. first_block[g + 1] - 1 (the last group: to the end of the grid): one lane per (query, column) of it.
//   planes  group g's columns, scalar (r, j) at planes + (j * stride + r) * 32
//   cols    its columns;  col_off: the columns of the groups before it (its place in a query's output row)
//   div     h_0 / h_g: query index i opens its row i / div
struct DmmcsRowParts {
    const uint8_t *planes[HADES252_MMCS_MAX_GROUPS];
    uint64_t stride[HADES252_MMCS_MAX_GROUPS];
    uint64_t col_off[HADES252_MMCS_MAX_GROUPS];
    uint32_t cols[HADES252_MMCS_MAX_GROUPS];
    uint32_t div[HADES252_MMCS_MAX_GROUPS];
    uint32_t first_block[HADES252_MMCS_MAX_GROUPS];
};

// rows[q][col_off_g + j] = M_g[indices[q] / div_g][j] for q < n, j < cols_g: the opened rows in the layout k_mmcs_verify
// reads (query-major, the groups concatenated tallest first).  The grid is the blocks of all groups laid end to end and a
// block finds its group from blockIdx.x alone, as in k_dmmcs_absorb, so the table lookup is scalar work.  Within a group
// the items run over (query, column) in output order: consecutive lanes write consecutive scalars of one query's row, and
// each loads its 32 bytes from its column's plane at that query's row.  The block's first item is split into (query,
// column) once per block (64-bit, uniform); a lane adds its offset with a 32-bit division (cols + 256 < 2^32), and the row
// is a 32-bit division too (index < h_0 <= 2^30): arity 3 needs a real one.  An index >= h_0 stores zeros and loads nothing.
__global__ void __launch_bounds__(kBlock, 3) k_dmmcs_rows(DmmcsRowParts parts, uint32_t n_parts, const uint64_t *__restrict__ indices,
                                                          size_t n, uint64_t h0, size_t row_cols, uint8_t *__restrict__ rows) {
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
        v = load_word(parts.planes[g] + ((size_t)j * parts.stride[g] + r) * 32);
    }
    store_word(rows + (q * row_cols + parts.col_off[g] + j) * 32, v);
}
