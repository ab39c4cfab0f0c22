// kernels_matrix.hpp -- row hashes of a matrix stored column by column: one row per lane, the sponge of kernels_sponge.hpp
// Part of the single translation unit hades252.hip (included there after kernels_inverse.hpp); not a stand-alone header.
#pragma once

// Scalar (r, c) of the matrix lies at planes + (c * stride + r) * 32: column c is one contiguous plane with one entry per
// row.  Lane r hashes row r = (M[r][0], ..., M[r][n_cols - 1]) exactly as k_sponge hashes a message of n_cols scalars: state
// [capacity, 0, 0, 0, 0]; every block of four columns is added into words 1..4 and followed by a permutation; pad_mode 1
// puts Montgomery one at position n_cols; positions past that contribute zero; at least one permutation; digest = word 1.
//   * loads: consecutive lanes own consecutive rows, so the two 16-byte loads of a lane cover, over the wave, 2 KiB
//     contiguous of the column.  Nothing goes through LDS on the way in (k_sponge re-tiles row-major messages there).
//   * every row has n_cols scalars: the trip count is a kernel argument's function, wave-uniform by construction -- no
//     shuffle reduction, no digest latch.
//   * the four columns of block t + 1 are requested before block t is permuted and are first used after it: the
//     permutation (about 2 000 dependent multiply-adds) hides their latency.
//   * a lane with row >= n_rows leaves at once: it reads nothing and writes nothing, and there is no barrier to miss.
//     No byte outside [c * stride, c * stride + n_rows) of any plane is read.
//   * digests leave as 32 contiguous bytes per lane (two 16-byte stores, 2 KiB contiguous over the wave): no LDS at all.

#ifndef HADES_MATRIX_MINW
#define HADES_MATRIX_MINW 3
#endif

// scalar (row, c) of the padded row: the matrix entry, Montgomery one at position n_cols (pad_mode 1), zero past it.
// c, n_cols and pad_mode are wave-uniform: the branch is one.
__device__ __forceinline__ Fr planes_word(const uint8_t *__restrict__ planes, size_t row, size_t stride, size_t n_cols,
                                          size_t c, int pad_mode) {
    if (c < n_cols) return load_word(planes + (c * stride + row) * 32);
    return fr_select(pad_mode == 1 && c == n_cols, one_mont_word(), zero_word());
}

// __launch_bounds__(256, 3): at least 3 waves per SIMD, i.e. at most 168 VGPRs -- the state, the four words in flight and
// the working set of fast_perm; no LDS, so registers alone decide the residency.
__global__ void __launch_bounds__(kBlock, HADES_MATRIX_MINW) k_sponge_planes(const uint8_t *__restrict__ planes, size_t n_rows,
                                                                             size_t n_cols, size_t stride,
                                                                             uint8_t *__restrict__ digests, Fr capacity,
                                                                             int pad_mode) {
    const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= n_rows) return;
    size_t blocks = (n_cols + (pad_mode == 1 ? 1 : 0) + 3) / 4;      // hades252_sponge_blocks(n_cols, pad_mode)
    if (blocks == 0) blocks = 1;
    Fr st[5];
    st[0] = capacity;
#pragma unroll
    for (int w = 1; w < 5; w++) st[w] = zero_word();
    Fr nxt[4];
#pragma unroll
    for (int k = 0; k < 4; k++) nxt[k] = planes_word(planes, row, stride, n_cols, (size_t)k, pad_mode);
#pragma unroll 1
    for (size_t t = 0; t < blocks; t++) {
#pragma unroll
        for (int k = 0; k < 4; k++) st[1 + k] = fr_add(st[1 + k], nxt[k]);
        if (t + 1 < blocks) {                                         // in flight during the permutation
#pragma unroll
            for (int k = 0; k < 4; k++) nxt[k] = planes_word(planes, row, stride, n_cols, 4 * (t + 1) + k, pad_mode);
        }
        Fr out[5];
        fast_perm<5>(&d_fast, st, out, 0);
#pragma unroll
        for (int w = 0; w < 5; w++) st[w] = out[w];
    }
    store_word(digests + row * 32, st[1]);
}
