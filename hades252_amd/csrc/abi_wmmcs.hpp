// abi_wmmcs.hpp -- C ABI, DEVICE memory in and out, on the caller's stream: gadget witnesses of the openings of a mixed-height
// commitment (kernels_wmmcs.hpp).  The shape rules, the group table and the closed-form count of a chain are host_mmcs.hpp's
// (mmcs_verify_shape); the wires are hades252_perm_witness_dev's.  Every call decides everything before it touches the
// device, enqueues on `stream` and returns: nothing is synchronised, nothing is downloaded (include/hades252.h, f17).
#pragma once

extern "C" {

// The shape of one opening as hades252_mmcs_verify checks it, or false: the one place the walk's count comes from.
static bool wmmcs_shape(const uint64_t *heights, const uint64_t *cols, size_t n_groups, int arity, int pad_mode, size_t n_queries,
                        MmcsShape &sh) {
    if (heights == nullptr || cols == nullptr || host_misaligned(heights) || host_misaligned(cols) || n_groups < 1 ||
        n_groups > HADES252_MMCS_MAX_GROUPS || arity < 2 || arity > 4 || (pad_mode != 0 && pad_mode != 1))
        return false;
    return mmcs_verify_shape(heights, cols, n_groups, arity, pad_mode, n_queries, sh);
}

size_t hades252_wmmcs_perms(const uint64_t *heights, const uint64_t *cols, size_t n_groups, int arity, int pad_mode) {
    MmcsShape sh;
    return wmmcs_shape(heights, cols, n_groups, arity, pad_mode, 1, sh) ? sh.n_perms : 0;
}

// The walk of k_mmcs_inputs as data, from the group table the launch passes: per group its blocks, its injection (g > 0) and
// the levels up to the next group's height.
int hades252_wmmcs_steps(const uint64_t *heights, const uint64_t *cols, size_t n_groups, int arity, int pad_mode, uint32_t *steps,
                         size_t n_steps) {
    MmcsShape sh;
    if (steps == nullptr || ((uintptr_t)steps & 3u) != 0 || !wmmcs_shape(heights, cols, n_groups, arity, pad_mode, 1, sh) ||
        n_steps != sh.n_perms)
        return HADES252_ERR_INVALID_ARG;
    uint32_t *at = steps, level = 0;
    for (uint32_t g = 0; g < (uint32_t)n_groups; g++) {
        const uint32_t blocks = (uint32_t)hades252_sponge_blocks(sh.table.cols[g], pad_mode);
        for (uint32_t b = 0; b < blocks; b++, at += 3) at[0] = HADES252_WMMCS_SPONGE, at[1] = g, at[2] = b;
        if (g > 0) {
            at[0] = HADES252_WMMCS_INJECT, at[1] = g, at[2] = 0;
            at += 3;
        }
        for (uint32_t l = 0; l < sh.table.climb[g]; l++, at += 3) at[0] = HADES252_WMMCS_CLIMB, at[1] = g, at[2] = level++;
    }
    return (size_t)(at - steps) == 3 * sh.n_perms ? HADES252_OK : HADES252_ERR_INVALID_ARG;
}

// ONE launch of k_mmcs_inputs over all queries, straight from the caller's buffers.
int hades252_wmmcs_inputs(const void *d_rows, const uint64_t *heights, const uint64_t *cols, size_t n_groups,
                          const uint64_t *d_indices, const void *d_paths, size_t n_queries, int arity,
                          const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                          const uint64_t inject_tag_mont[4], int out_idx, void *d_inputs, void *d_roots, void *stream) {
    if (n_queries == 0) return HADES252_OK;
    if (d_rows == nullptr || d_indices == nullptr || d_paths == nullptr || d_inputs == nullptr || capacity_mont == nullptr ||
        tag_mont == nullptr || inject_tag_mont == nullptr || misaligned(d_rows) || host_misaligned(d_indices) || misaligned(d_paths) ||
        misaligned(d_inputs) || misaligned(d_roots) || out_idx < 0 || out_idx >= 5 || n_queries > kMaxLaunchRecords)
        return HADES252_ERR_INVALID_ARG;
    MmcsShape sh;
    if (!wmmcs_shape(heights, cols, n_groups, arity, pad_mode, n_queries, sh) || sh.n_perms > kMaxLaunchRecords / n_queries)
        return HADES252_ERR_INVALID_ARG;
    const int rc = check_device();
    if (rc != HADES252_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Fr cap = fr_from_u64(capacity_mont), tag = fr_from_u64(tag_mont), inject_tag = fr_from_u64(inject_tag_mont);
    const MmcsGroups &table = sh.table;
    const size_t row_cols = sh.row_cols, n_perms = sh.n_perms;
    const uint32_t depth = (uint32_t)sh.depth;
    const uint64_t *d_idx = d_indices;
#define HADES_LAUNCH_MMCS_INPUTS(A)                                                                                                 \
    hipLaunchKernelGGL(k_mmcs_inputs<A>, dim3(blocks_for(n_queries)), dim3(kBlock), 0, s, (const uint8_t *)d_rows, d_idx,             \
                       (const uint8_t *)d_paths, n_queries, table, (uint32_t)n_groups, row_cols, depth, n_perms, pad_mode, cap, tag, \
                       inject_tag, out_idx, (uint8_t *)d_inputs, (uint8_t *)d_roots)
    switch (arity) {
        case 2: HADES_LAUNCH_MMCS_INPUTS(2); break;
        case 3: HADES_LAUNCH_MMCS_INPUTS(3); break;
        default: HADES_LAUNCH_MMCS_INPUTS(4); break;
    }
#undef HADES_LAUNCH_MMCS_INPUTS
    HIP_TRY(hipGetLastError());
    return HADES252_OK;
}

// The inputs stage, then the independent records through k_perm_witness on the same stream: wires == perm_witness(inputs) by
// construction.
int hades252_wmmcs_witness(const void *d_rows, const uint64_t *heights, const uint64_t *cols, size_t n_groups,
                           const uint64_t *d_indices, const void *d_paths, size_t n_queries, int arity,
                           const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                           const uint64_t inject_tag_mont[4], int out_idx, void *d_inputs, void *d_wires, void *d_roots,
                           void *stream) {
    if (n_queries == 0) return HADES252_OK;
    if (d_wires == nullptr || misaligned(d_wires)) return HADES252_ERR_INVALID_ARG;
    const int rc = hades252_wmmcs_inputs(d_rows, heights, cols, n_groups, d_indices, d_paths, n_queries, arity, capacity_mont, pad_mode,
                                         tag_mont, inject_tag_mont, out_idx, d_inputs, d_roots, stream);
    if (rc != HADES252_OK) return rc;
    return hades252_perm_witness_dev(d_inputs, d_wires, hades252_wmmcs_perms(heights, cols, n_groups, arity, pad_mode) * n_queries, stream);
}

}  // extern "C"
