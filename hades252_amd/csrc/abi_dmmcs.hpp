// abi_dmmcs.hpp -- C ABI, DEVICE memory in and out, on the caller's stream: the mixed-height commitments of host_mmcs.hpp fed,
// opened and verified without a copy (kernels_dmmcs.hpp).  The handle is hades252_mmcs_new's; commit and free stay
// host_mmcs.hpp's.  Every call decides everything before it touches the device, enqueues on `stream` and returns: nothing is
// synchronised, nothing is downloaded.  The library orders nothing between the caller's stream and its own pipe streams: the
// caller synchronises its stream before a host-form call on the same handle (include/hades252.h, f15).
#pragma once

extern "C" {

// Parts of one absorb in the grid, shortest first: a short group's blocks are a chain of as many permutations as the tall
// group's, so they start first and run beside it.  Test hook: HADES252_TEST_DMMCS_TALL_FIRST (read once, at the first call;
// any value but 0) lays them tallest first instead, for the A/B of tools/time_dmmcs.py.
static bool dmmcs_tall_first() {
    static const bool forced = []() -> bool {
        const char *e = getenv("HADES252_TEST_DMMCS_TALL_FIRST");
        return e != nullptr && strtoull(e, nullptr, 0) != 0;
    }();
    return forced;
}

int hades252_dmmcs_absorb(void *mc, const void *const *d_planes, const uint64_t *n_rows, const uint64_t *n_cols,
                          const uint64_t *plane_strides, size_t n_parts, void *stream) {
    MmcsHandle *h = (MmcsHandle *)mc;
    if (h == nullptr || d_planes == nullptr || n_rows == nullptr || n_cols == nullptr || plane_strides == nullptr || n_parts < 1 ||
        n_parts > HADES252_MMCS_MAX_GROUPS)
        return HADES252_ERR_INVALID_ARG;
    int live[HADES252_MMCS_MAX_GROUPS], n_live = 0, n_new = 0;         // the parts with columns, in the order of the grid
    for (size_t p = 0; p < n_parts; p++) {
        if (n_cols[p] == 0) continue;
        if (n_rows[p] == 0 || n_rows[p] > kMaxLaunchRecords || d_planes[p] == nullptr || misaligned(d_planes[p]) ||
            plane_strides[p] < n_rows[p] || plane_strides[p] > SIZE_MAX / 32 / n_cols[p])
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
    DmmcsParts table = {};
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
        table.planes[i] = (const uint8_t *)d_planes[p];
        table.state[i] = ms->d_state;
        table.S[i] = n_rows[p];
        table.stride[i] = plane_strides[p];
        table.g[i] = n_cols[p];
        table.first_block[i] = (uint32_t)n_blocks;
        table.cur[i] = (uint32_t)(ms->n_cols % 4);
        n_blocks += blocks_for((size_t)n_rows[p]);                     // (at most 32 x 2^22 blocks)
    }
    hipLaunchKernelGGL(k_dmmcs_absorb, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (uint32_t)n_live);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        tl_last_hip_error = (int)e;
        h->poisoned = true;
        return HADES252_ERR_HIP;
    }
    for (int i = 0; i < n_live; i++) groups[i]->n_cols += n_cols[live[i]];
    return HADES252_OK;
}

int hades252_dmmcs_tree(const void *mc, const void **d_tree, size_t *tree_bytes, int *arity) {
    const MmcsHandle *h = (const MmcsHandle *)mc;
    if (h == nullptr || d_tree == nullptr || tree_bytes == nullptr || arity == nullptr || h->tree_rows == 0)
        return HADES252_ERR_INVALID_ARG;
    if (h->poisoned) return HADES252_ERR_HIP;
    *d_tree = h->d_tree;
    *tree_bytes = hades252_mmcs_tree_bytes(h->tree_rows, h->tree_arity);
    *arity = h->tree_arity;
    return HADES252_OK;
}

int hades252_dmmcs_open(const void *mc, const void *const *d_planes, const uint64_t *n_rows, const uint64_t *n_cols,
                        const uint64_t *plane_strides, size_t n_parts, const uint64_t *d_indices, size_t n_queries,
                        void *d_rows, void *d_paths, void *stream) {
    MmcsHandle *h = (MmcsHandle *)mc;                                  // (a failed launch poisons it: nothing else is written)
    if (h == nullptr) return HADES252_ERR_INVALID_ARG;
    if (n_queries == 0) return h->poisoned ? HADES252_ERR_HIP : HADES252_OK;
    if (d_planes == nullptr || n_rows == nullptr || n_cols == nullptr || plane_strides == nullptr || n_parts < 1 ||
        n_parts > HADES252_MMCS_MAX_GROUPS || d_indices == nullptr || d_rows == nullptr || d_paths == nullptr ||
        host_misaligned(d_indices) || misaligned(d_rows) || misaligned(d_paths) || n_queries > kMaxLaunchRecords ||
        h->tree_rows == 0 || n_rows[0] != h->tree_rows)
        return HADES252_ERR_INVALID_ARG;
    const size_t h0 = h->tree_rows;
    const int arity = h->tree_arity, depth = mmcs_log(h0, arity);
    DmmcsRowParts table = {};
    size_t row_cols = 0;
    uint64_t n_blocks = 0;                                             // (at most 32 x 2^22)
    for (size_t p = 0; p < n_parts; p++) {
        if ((p > 0 && n_rows[p] >= n_rows[p - 1]) || n_rows[p] == 0 || h0 % n_rows[p] != 0 || mmcs_group(h, (size_t)n_rows[p]) == nullptr ||
            n_cols[p] < 1 || n_cols[p] > kMaxLaunchRecords || n_queries > kMaxLaunchRecords / n_cols[p] || d_planes[p] == nullptr ||
            misaligned(d_planes[p]) || plane_strides[p] < n_rows[p] || plane_strides[p] > SIZE_MAX / 32 / n_cols[p])
            return HADES252_ERR_INVALID_ARG;
        table.planes[p] = (const uint8_t *)d_planes[p];
        table.stride[p] = plane_strides[p];
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
    hipLaunchKernelGGL(k_dmmcs_rows, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (uint32_t)n_parts, d_indices,
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

// ONE launch of k_mmcs_verify over all queries, straight from the caller's buffers: no chunks, no pipe, no copy.
int hades252_dmmcs_verify(const void *d_rows, const uint64_t *heights, const uint64_t *cols, size_t n_groups,
                          const uint64_t *d_indices, const void *d_paths, size_t n_queries, int arity,
                          const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                          const uint64_t inject_tag_mont[4], int out_idx, void *d_roots, void *stream) {
    if (n_queries == 0) return HADES252_OK;
    if (d_rows == nullptr || heights == nullptr || cols == nullptr || d_indices == nullptr || d_paths == nullptr || d_roots == nullptr ||
        capacity_mont == nullptr || tag_mont == nullptr || inject_tag_mont == nullptr || misaligned(d_rows) ||
        host_misaligned(heights) || host_misaligned(cols) || host_misaligned(d_indices) || misaligned(d_paths) ||
        misaligned(d_roots) || n_groups < 1 || n_groups > HADES252_MMCS_MAX_GROUPS || arity < 2 || arity > 4 ||
        (pad_mode != 0 && pad_mode != 1) || out_idx < 0 || out_idx >= 5 || n_queries > kMaxLaunchRecords)
        return HADES252_ERR_INVALID_ARG;
    MmcsShape sh;
    if (!mmcs_verify_shape(heights, cols, n_groups, arity, pad_mode, n_queries, sh)) return HADES252_ERR_INVALID_ARG;
    const int rc = check_device();
    if (rc != HADES252_OK) return rc;
    mmcs_launch_verify(arity, (hipStream_t)stream, (const uint8_t *)d_rows, d_indices, (const uint8_t *)d_paths, n_queries, sh.table,
                       (uint32_t)n_groups, sh.row_cols, (uint32_t)sh.depth, sh.n_perms, pad_mode, fr_from_u64(capacity_mont),
                       fr_from_u64(tag_mont), fr_from_u64(inject_tag_mont), out_idx, (uint8_t *)d_roots);
    HIP_TRY(hipGetLastError());
    return HADES252_OK;
}

}  // extern "C"
