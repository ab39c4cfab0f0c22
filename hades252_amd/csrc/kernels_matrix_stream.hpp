// kernels_matrix_stream.hpp -- the row sponges of kernels_matrix.hpp kept RESIDENT between launches: a matrix stored column
// by column is taken a group of columns at a time, over all rows, and finished at any point (host_matrix_stream.hpp).
// Part of the single translation unit hades252.hip (included there after kernels_matrix.hpp); not a stand-alone header.
#pragma once

// The state of row r is the five-word sponge state of k_sponge_planes after c columns: floor(c / 4) blocks added into words
// 1..4 and permuted, the c % 4 columns of the open block added and NOT permuted.  It lives in five planes: word w of row r
// lies at state + (w * S + r) * 32, S the plane stride (the matrix's row count).
//   * one row per lane, consecutive lanes own consecutive rows: a wave's two 16-byte loads (or stores) of a state word
//     cover 2 KiB contiguous, as its loads of a column do.  Nothing goes through LDS: the array-of-states format of
//     k_sponge_absorb (160 bytes per state) would need its re-tiling, which is why it is not used here.
//   * every branch depends on kernel arguments only and is wave-uniform; the state words are indexed by unrolled constants
//     (a run-time index would put the state into scratch).
//   * a lane with row >= m leaves at once: it reads nothing and writes nothing, and there is no barrier to miss.  No byte
//     outside rows [0, m) of any column plane or state plane is touched.
//   * registers: the state, the four words in flight and the working set of fast_perm, as k_sponge_planes; no LDS, no
//     scratch, so registers alone decide the residency.

#ifndef HADES_MATRIX_STREAM_MINW
#define HADES_MATRIX_STREAM_MINW 3
#endif

// state[r] = [capacity, 0, 0, 0, 0] for rows [0, m): a fresh sponge
__global__ void __launch_bounds__(kBlock, HADES_MATRIX_STREAM_MINW) k_planes_init(uint8_t *__restrict__ state, size_t S, size_t m,
                                                                                  Fr capacity) {
    const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= m) return;
    store_word(state + row * 32, capacity);
#pragma unroll
    for (int w = 1; w < 5; w++) store_word(state + ((size_t)w * S + row) * 32, zero_word());
}

// Rows [0, m) absorb columns 0 .. g - 1 of `planes` (scalar (r, j) at planes + (j * stride + r) * 32); `cur` = columns
// already in the open block (the stream's column total mod 4).
//   head   up to 4 - cur columns complete the open block: adds only, and a permutation if the block closes;
//   body   whole blocks of four: the four columns of block t + 1 are requested before block t is permuted and are first
//          used after it (the pattern of k_sponge_planes: the permutation hides their latency);
//   tail   fewer than four columns open a new block: adds only.
__global__ void __launch_bounds__(kBlock, HADES_MATRIX_STREAM_MINW) k_planes_absorb(uint8_t *__restrict__ state, size_t S, size_t m,
                                                                                    const uint8_t *__restrict__ planes, size_t g,
                                                                                    size_t stride, int cur) {
    const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= m) return;
    Fr st[5];
#pragma unroll
    for (int w = 0; w < 5; w++) st[w] = load_word(state + ((size_t)w * S + row) * 32);
    size_t c = 0;                                                     // columns of the group taken so far
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

// digests[r] = what k_sponge_planes gives for the columns absorbed so far: under pad_mode 1 Montgomery one joins the open
// block at position `open` (the column total mod 4); a permutation if open != 0 or pad_mode == 1; word 1.  The state is
// only read, so the stream can go on absorbing.  Where no permutation is due (whole blocks, pad_mode 0) word 1 alone is
// loaded.
__global__ void __launch_bounds__(kBlock, HADES_MATRIX_STREAM_MINW) k_planes_finish(const uint8_t *__restrict__ state, size_t S,
                                                                                    size_t m, uint8_t *__restrict__ digests,
                                                                                    int open, int pad_mode) {
    const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= m) return;
    if (open == 0 && pad_mode != 1) {
        store_word(digests + row * 32, load_word(state + (S + row) * 32));
        return;
    }
    Fr st[5];
#pragma unroll
    for (int w = 0; w < 5; w++) st[w] = load_word(state + ((size_t)w * S + row) * 32);
    if (pad_mode == 1) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k == open) st[1 + k] = fr_add(st[1 + k], one_mont_word());
    }
    Fr out[5];
    fast_perm<5>(&d_fast, st, out, 0);
    store_word(digests + row * 32, out[1]);
}
