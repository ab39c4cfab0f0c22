// host_rowmajor.hpp -- C ABI, HOST memory in: a row-major matrix into a mixed-height commitment (host_mmcs.hpp), without a
// transpose anywhere.  The matrix travels in the tiles of host_matrix_stream.hpp -- K rows x G columns, two device buffers,
// tile t + 1 copied while tile t is absorbed -- but a tile lands row-major in its buffer (one pitched 2-D copy: K pieces of
// G * 32 bytes, source pitch row_stride * 32) and is absorbed by k_rm_absorb (kernels_rowmajor.hpp) as a one-part table.
#pragma once

extern "C" {

// Tile t (buffer t % 2, at d) of m rows x gw columns from `from`, before its launch: matrix_tile_in's place in the pipeline
// with a row-major tile.  The buffer's row stride is gw, so a tile of whole rows of a matrix without a gap (gw ==
// row_stride) is ONE contiguous copy.
static int rm_tile_in(HostCall &call, size_t t, uint8_t *d, const uint64_t *from, size_t row_stride, size_t m, size_t gw) {
    HostPipe &pp = call.pipe;
    const int k = (int)(t % 2);
    if (t >= 2) TRY_CALL(call, F(F_SYNC, hipEventSynchronize(pp.k_done[k])));         // tile t - 2 is done: buffer k is free
    if (gw == row_stride)
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d, from, m * gw * 32, hipMemcpyHostToDevice, pp.s_in)));
    else
        TRY_CALL(call, F(F_MEMCPY, hipMemcpy2DAsync(d, gw * 32, from, row_stride * 32, gw * 32, m, hipMemcpyHostToDevice, pp.s_in)));
    TRY_CALL(call, hipEventRecord(pp.in_done[k], pp.s_in));
    TRY_CALL(call, hipStreamWaitEvent(pp.s_k, pp.in_done[k], 0));
    return HADES252_OK;
}

// mstream_absorb_tiles for a row-major matrix: the same K and G (and their test hooks), the same shortened first column tile,
// the same order -- column tiles outside, row tiles inside, all kernels on the kernel stream.
static int rm_absorb_tiles(MatrixStreamHandle *ms, const uint64_t *rows, size_t n_cols, size_t row_stride) {
    const size_t S = ms->n_rows;
    const size_t K = matrix_tile_rows(1, S);                           // the test hook's value, else kMatrixFullRows
    size_t G = mstream_forced_cols();
    if (G == 0) G = kMatrixTargetBytes / (32 * K);
    if (G < 1) G = 1;
    if (G >= 4) G -= G % 4;
    if (G > n_cols) G = n_cols;
    const bool align = G % 4 == 0 && G < n_cols;                       // several tiles of whole blocks: (G >= 4 > cur)
    const size_t buf_b = up256(K * G * 32);
    HostCall call;
    int rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    rc = pipe_ensure_aux(pp, 2 * buf_b);
    if (rc != HADES252_OK) return call.finish(rc);
    RmParts table = {};
    table.S[0] = S;
    table.col_step[0] = 1;
    size_t t = 0;
    unsigned cur = (unsigned)(ms->n_cols % 4);
    for (size_t j = 0; j < n_cols;) {
        size_t gw = j == 0 && align ? G - cur : G;
        if (gw > n_cols - j) gw = n_cols - j;
        for (size_t off = 0; off < S; off += K, t++) {
            const size_t m = S - off < K ? S - off : K;
            uint8_t *d = (uint8_t *)pp.aux + t % 2 * buf_b;
            rc = rm_tile_in(call, t, d, rows + (off * row_stride + j) * 4, row_stride, m, gw);
            if (rc != HADES252_OK) return rc;
            table.base[0] = d;
            table.state[0] = ms->d_state + off * 32;
            table.rows[0] = m;
            table.row_step[0] = gw;
            table.g[0] = gw;
            table.cur[0] = cur;
            hipLaunchKernelGGL(k_rm_absorb, dim3(blocks_for(m)), dim3(kBlock), 0, pp.s_k, table, 1u);
            rc = matrix_tile_launched(call, t);
            if (rc != HADES252_OK) return rc;
        }
        j += gw;
        cur = (unsigned)((cur + gw) % 4);
    }
    TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(pp.s_k)));           // the caller may reuse `rows`
    return call.finish(HADES252_OK);
}

int hades252_rmmcs_absorb_rows(void *mc, const uint64_t *rows, size_t n_rows, size_t n_cols, size_t row_stride) {
    MmcsHandle *h = (MmcsHandle *)mc;
    if (h == nullptr) return HADES252_ERR_INVALID_ARG;
    if (n_cols == 0) return h->poisoned ? HADES252_ERR_HIP : HADES252_OK;
    if (n_rows == 0 || n_rows > kMaxLaunchRecords || rows == nullptr || host_misaligned(rows) || row_stride < n_cols ||
        row_stride > SIZE_MAX / 32 / n_rows)
        return HADES252_ERR_INVALID_ARG;
    MatrixStreamHandle *ms = mmcs_group(h, n_rows);
    if (ms == nullptr ? h->n_groups == HADES252_MMCS_MAX_GROUPS : (uint64_t)n_cols > UINT64_MAX - ms->n_cols)
        return HADES252_ERR_INVALID_ARG;
    int rc = mmcs_enter(h);
    if (rc != HADES252_OK) return rc;
    if (ms == nullptr) {
        rc = mmcs_poison_on_hip(h, mmcs_add_group(h, n_rows, &ms));
        if (rc != HADES252_OK) return rc;
    }
    rc = mmcs_poison_on_hip(h, rm_absorb_tiles(ms, rows, n_cols, row_stride));
    if (rc == HADES252_OK) ms->n_cols += n_cols;
    return rc;
}

}  // extern "C"
