// abi_rowmajor.hpp -- C ABI, DEVICE memory in and out, on the caller's stream: the device-resident mixed-height commitments of
// abi_dmmcs.hpp with a layout per matrix, column-major or row-major (kernels_rowmajor.hpp).  The handle, its groups and the
// order of the grid are abi_dmmcs.hpp's and host_mmcs.hpp's; hades252_dmmcs_absorb and hades252_dmmcs_open keep their own
// kernels.  As there: every call decides everything before it touches the device, enqueues on `stream` and returns.
#pragma once

extern "C" {

// The two steps of a matrix of n_rows x n_cols scalars with `stride` in its layout (kernels_rowmajor.hpp), or false: a
// layout that is none, a stride below the extent it strides over, a byte count beyond size_t.  (n_rows, n_cols >= 1)
static bool rm_steps(uint32_t layout, uint64_t n_rows, uint64_t n_cols, uint64_t stride, uint64_t *row_step, uint64_t *col_step) {
    if (layout == HADES252_LAYOUT_COLS) {
        if (stride < n_rows || stride > SIZE_MAX / 32 / n_cols) return false;
        *row_step = 1;
        *col_step = stride;
        return true;
    }
    if (layout != HADES252_LAYOUT_ROWS || stride < n_cols || stride > SIZE_MAX / 32 / n_rows) return false;
    *row_step = stride;
    *col_step = 1;
    return true;
}

int hades252_rmmcs_absorb_ex(void *mc, const void *const *d_mats, const uint64_t *n_rows, const uint64_t *n_cols,
                             const uint64_t *strides, const uint32_t *layouts, size_t n_parts, void *stream) {
    MmcsHandle *h = (MmcsHandle *)mc;
    if (h == nullptr || d_mats == nullptr || n_rows == nullptr || n_cols == nullptr || strides == nullptr || n_parts < 1 ||
        n_parts > HADES252_MMCS_MAX_GROUPS)
        return HADES252_ERR_INVALID_ARG;
    int live[HADES252_MMCS_MAX_GROUPS], n_live = 0, n_new = 0;         // the parts with columns, in the order of the grid
    uint64_t row_step[HADES252_MMCS_MAX_GROUPS], col_step[HADES252_MMCS_MAX_GROUPS];   // by part
    for (size_t p = 0; p < n_parts; p++) {
        if (n_cols[p] == 0) continue;
        if (n_rows[p] == 0 || n_rows[p] > kMaxLaunchRecords || d_mats[p] == nullptr || misaligned(d_mats[p]) ||
            !rm_steps(layouts != nullptr ? layouts[p] : HADES252_LAYOUT_COLS, n_rows[p], n_cols[p], strides[p], &row_step[p], &col_step[p]))
            return HADES252_ERR_INVALID_ARG;
        for (int i = 0; i < n_live; i++)
            if (n_rows[live[i]] == n_rows[p]) return HADES252_ERR_INVALID_ARG;
        const MatrixStreamHandle *ms = mmcs_group(h, (size_t)n_rows[p]);
        if (ms == nullptr ? h->n_groups + ++n_new > HADES252_MMCS_MAX_GROUPS : n_cols[p] > UINT64_MAX - ms->n_cols)
            return HADES252_ERR_INVALID_ARG;
        int i = n_live++;                                              // by rising height (falling, under the test hook)
        for (; i > 0 && (n_rows[live[i - 1]] > n_rows[p]) != dmmcs_tall_first(); i--) live[i] = live[i - 1];
        live[i] = (int)p;
    }
    if (n_live == 0) return h->poisoned ? HADES252_ERR_HIP : HADES252_OK;
    int rc = mmcs_enter(h);
    if (rc != HADES252_OK) return rc;
    RmParts table = {};
    MatrixStreamHandle *groups[HADES252_MMCS_MAX_GROUPS];
    uint64_t n_blocks = 0;
    for (int i = 0; i < n_live; i++) {
        const int p = live[i];
        MatrixStreamHandle *ms = mmcs_group(h, (size_t)n_rows[p]);
        if (ms == nullptr) {                                           // (its state planes are initialised when this returns)
            rc = mmcs_poison_on_hip(h, mmcs_add_group(h, (size_t)n_rows[p], &ms));
            if (rc != HADES252_OK) return rc;
        }
        groups[i] = ms;
        table.base[i] = (const uint8_t *)d_mats[p];
        table.state[i] = ms->d_state;
        table.S[i] = n_rows[p];
        table.rows[i] = n_rows[p];
        table.row_step[i] = row_step[p];
        table.col_step[i] = col_step[p];
        table.g[i] = n_cols[p];
        table.first_block[i] = (uint32_t)n_blocks;
        table.cur[i] = (uint32_t)(ms->n_cols % 4);
        n_blocks += blocks_for((size_t)n_rows[p]);                     // (at most 32 x 2^22 blocks)
    }
    hipLaunchKernelGGL(k_rm_absorb, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (uint32_t)n_live);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        tl_last_hip_error = (int)e;
        h->poisoned = true;
        return HADES252_ERR_HIP;
    }
    for (int i = 0; i < n_live; i++) groups[i]->n_cols += n_cols[live[i]];
    return HADES252_OK;
}

int hades252_rmmcs_open_ex(const void *mc, const void *const *d_mats, const uint64_t *n_rows, const uint64_t *n_cols,
                           const uint64_t *strides, const uint32_t *layouts, size_t n_parts, const uint64_t *d_indices,
                           size_t n_queries, void *d_rows, void *d_paths, void *stream) {
    MmcsHandle *h = (MmcsHandle *)mc;                                  // (a failed launch poisons it: nothing else is written)
    if (h == nullptr) return HADES252_ERR_INVALID_ARG;
    if (n_queries == 0) return h->poisoned ? HADES252_ERR_HIP : HADES252_OK;
    if (d_mats == nullptr || n_rows == nullptr || n_cols == nullptr || strides == nullptr || n_parts < 1 ||
        n_parts > HADES252_MMCS_MAX_GROUPS || d_indices == nullptr || d_rows == nullptr || d_paths == nullptr ||
        host_misaligned(d_indices) || misaligned(d_rows) || misaligned(d_paths) || n_queries > kMaxLaunchRecords ||
        h->tree_rows == 0 || n_rows[0] != h->tree_rows)
        return HADES252_ERR_INVALID_ARG;
    const size_t h0 = h->tree_rows;
    const int arity = h->tree_arity, depth = mmcs_log(h0, arity);
    RmRowParts table = {};
    size_t row_cols = 0;
    uint64_t n_blocks = 0;                                             // (at most 32 x 2^22)
    for (size_t p = 0; p < n_parts; p++) {
        if ((p > 0 && n_rows[p] >= n_rows[p - 1]) || n_rows[p] == 0 || h0 % n_rows[p] != 0 || mmcs_group(h, (size_t)n_rows[p]) == nullptr ||
            n_cols[p] < 1 || n_cols[p] > kMaxLaunchRecords || n_queries > kMaxLaunchRecords / n_cols[p] || d_mats[p] == nullptr ||
            misaligned(d_mats[p]) ||
            !rm_steps(layouts != nullptr ? layouts[p] : HADES252_LAYOUT_COLS, n_rows[p], n_cols[p], strides[p], &table.row_step[p],
                      &table.col_step[p]))
            return HADES252_ERR_INVALID_ARG;
        table.base[p] = (const uint8_t *)d_mats[p];
        table.col_off[p] = row_cols;
        table.cols[p] = (uint32_t)n_cols[p];
        table.div[p] = (uint32_t)(h0 / n_rows[p]);
        table.first_block[p] = (uint32_t)n_blocks;
        row_cols += (size_t)n_cols[p];
        n_blocks += blocks_for(n_queries * (size_t)n_cols[p]);
    }
    if (n_queries > SIZE_MAX / 32 / row_cols || n_queries * (size_t)depth * (arity - 1) * 2 > kMaxLaunchRecords)
        return HADES252_ERR_INVALID_ARG;
    int rc = mmcs_enter(h);
    if (rc != HADES252_OK) return rc;
    hipLaunchKernelGGL(k_rm_rows, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (uint32_t)n_parts, d_indices,
                       n_queries, (uint64_t)h0, row_cols, (uint8_t *)d_rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        tl_last_hip_error = (int)e;
        h->poisoned = true;
        return HADES252_ERR_HIP;
    }
    // the tree's first level is the leaves of hades252_merkle_open_dev, what follows it the tree (host_mmcs.hpp)
    return mmcs_poison_on_hip(h, hades252_merkle_open_dev(h->d_tree, h->d_tree + h0 * 32, h0, arity, d_indices, n_queries, d_paths, stream));
}

}  // extern "C"
