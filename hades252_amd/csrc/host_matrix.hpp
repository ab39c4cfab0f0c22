// host_matrix.hpp -- C ABI, HOST memory in and out: commitments to a matrix stored column by column (kernels_matrix.hpp):
// the row digests, the Merkle tree over them, openings (plain host code) and batched verification.  A block of a row is 128
// bytes in for one permutation and the digests stay on the device between the hashing and the tree, so the copies are
// expected to hide behind the kernel and there is no device-pointer form.
#pragma once

extern "C" {

// Bytes of one chunk of rows, all columns together.  The chunk is what one 2-D copy moves and one launch hashes; two of
// them are resident.  What decides is ROWS, not bytes: a chunk's kernel runs one row per lane and every lane walks all of
// its blocks, so a launch takes blocks x one permutation latency (about 175 us) however few rows it has, and the chunks'
// kernels follow each other on one stream.  Measured (profiles/f12_matrix/README.md, 2^20 rows, 4 .. 128 MiB): the call's
// time is the number of chunks x that latency until a chunk's copy takes as long -- 64 columns (17 blocks): 1563 ms at
// 4 MiB, 199 ms at 32 MiB, 53 ms at 128 MiB, where the 3.3 ms per chunk are the link's 40 GB/s; 16 columns: 118 ms at
// 4 MiB, 16.7 / 15.8 / 17.0 ms at 32 / 64 / 128 MiB.  128 MiB is the smallest size at which 64 columns are bound by the
// link; two such buffers are 256 MiB of device memory.
static constexpr size_t kMatrixTargetBytes = (size_t)128 << 20;
// ... and no more rows than fill the device (256 CUs x 4 SIMDs x 3 waves x 64 lanes = 196 608, as a power of two): beyond
// that a larger chunk hashes no faster and only lengthens the first copy, which nothing overlaps (4 columns, 2^20 rows:
// see the same file for one chunk of 2^20 rows against four of 2^18).
static constexpr size_t kMatrixFullRows = (size_t)1 << 18;
// Rows per chunk of a matrix of n_rows rows: a multiple of 256 (whole blocks), at least 256 -- with
// HADES252_MATRIX_MAX_COLS columns that is 32 MiB -- and no more than the matrix has.
// Test hook: HADES252_TEST_MATRIX_CHUNK_ROWS (read once, at the first call) sets it, rounded down to a multiple of 256, so
// that a matrix of a thousand rows runs through several chunks (tests/test_gpu_f12_matrix.py) and the chunk size can be
// A/B-ed (tools/time_matrix.py); values below 256 are ignored.
static size_t matrix_tile_rows(size_t n_cols, size_t n_rows) {
    static const size_t forced = []() -> size_t {
        const char *e = getenv("HADES252_TEST_MATRIX_CHUNK_ROWS");
        const size_t t = e ? (size_t)strtoull(e, nullptr, 0) : 0;
        return t >= 256 ? t / 256 * 256 : 0;
    }();
    const size_t k = kMatrixTargetBytes / (32 * n_cols) / 256 * 256, all = (n_rows + 255) / 256 * 256;
    const size_t K = forced ? forced : k < 256 ? 256 : (k > kMatrixFullRows ? kMatrixFullRows : k);
    return K > all ? all : K;
}

static inline bool host_misaligned(const void *p) { return ((uintptr_t)p & 7u) != 0; }
static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the rules every call that reads the planes shares (n_rows > 0)
static bool matrix_shape_ok(const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride) {
    return planes != nullptr && !host_misaligned(planes) && n_cols >= 1 && n_cols <= HADES252_MATRIX_MAX_COLS &&
           plane_stride >= n_rows && n_rows <= kMaxLaunchRecords && plane_stride <= SIZE_MAX / 32 / n_cols;
}

// The two-buffer pipeline around the launch of tile t, whose buffer (t % 2) is d: the tile travels (one 2-D copy: `cols`
// pieces of m * 32 bytes, source pitch stride * 32, into a buffer whose plane stride is K) on the copy stream while tile
// t - 1 runs on the kernel stream; the host runs at most two tiles ahead.  matrix_tile_in comes before the launch,
// matrix_tile_launched after it; a failure of either has finished the call and the caller returns the code.  From memory
// that is not page-locked the runtime stages the 2-D copies itself and they do not overlap the kernel.
static int matrix_tile_in(HostCall &call, size_t t, uint8_t *d, size_t K, const uint64_t *from, size_t stride, size_t m, size_t cols) {
    HostPipe &pp = call.pipe;
    const int k = (int)(t % 2);
    if (t >= 2) TRY_CALL(call, F(F_SYNC, hipEventSynchronize(pp.k_done[k])));         // tile t - 2 is done: buffer k is free
    TRY_CALL(call, F(F_MEMCPY, hipMemcpy2DAsync(d, K * 32, from, stride * 32, m * 32, cols, hipMemcpyHostToDevice, pp.s_in)));
    TRY_CALL(call, hipEventRecord(pp.in_done[k], pp.s_in));
    TRY_CALL(call, hipStreamWaitEvent(pp.s_k, pp.in_done[k], 0));
    return HADES252_OK;
}
static int matrix_tile_launched(HostCall &call, size_t t) {
    TRY_CALL(call, hipGetLastError());
    TRY_CALL(call, hipEventRecord(call.pipe.k_done[t % 2], call.pipe.s_k));
    return HADES252_OK;
}

// Rows -> digests, a tile of K rows (all columns) at a time; the digests accumulate in d_dig (n_rows * 32 bytes, device).
static int matrix_hash_rows(HostCall &call, uint8_t *d_buf, size_t K, const uint64_t *planes, size_t n_rows, size_t n_cols,
                            size_t plane_stride, const uint64_t capacity_mont[4], int pad_mode, uint8_t *d_dig) {
    HostPipe &pp = call.pipe;
    const size_t buf_b = up256(K * n_cols * 32), n_chunks = (n_rows + K - 1) / K;
    const Fr cap = fr_from_u64(capacity_mont);
    for (size_t c = 0; c < n_chunks; c++) {
        const size_t off = c * K, m = n_rows - off < K ? n_rows - off : K;
        uint8_t *d = d_buf + c % 2 * buf_b;
        int rc = matrix_tile_in(call, c, d, K, planes + off * 4, plane_stride, m, n_cols);
        if (rc != HADES252_OK) return rc;
        hipLaunchKernelGGL(k_sponge_planes, dim3(blocks_for(m)), dim3(kBlock), 0, pp.s_k, d, m, n_cols, K, d_dig + off * 32, cap, pad_mode);
        rc = matrix_tile_launched(call, c);
        if (rc != HADES252_OK) return rc;
    }
    return HADES252_OK;
}

// The end of a commitment, one-shot or streamed, and of its call: the tree over the n_rows digests at d_dig into d_tree
// (d_pad: the uploaded padding table or NULL; the digests never leave the device in between), then what the caller asked
// for -- digests (may be NULL), tree (may be NULL) and root (NULL: no tree at all).
static int matrix_finish(HostCall &call, const uint8_t *d_dig, size_t n_rows, int arity, const uint64_t tag_mont[4], int out_idx,
                         const uint8_t *d_pad, uint8_t *d_tree, uint64_t *digests, uint64_t *tree, uint64_t *root) {
    HostPipe &pp = call.pipe;
    uint64_t got[4];                                                   // the caller's root is written on success only
    if (root != nullptr) {
        const size_t tree_bytes = hades252_merkle_tree_bytes(n_rows, arity);
        const int rc = hades252_merkle_build_pad_dev(d_dig, n_rows, arity, tag_mont, out_idx, d_pad, d_tree, pp.s_k);
        if (rc != HADES252_OK) return call.finish(rc);
        if (tree != nullptr)
            TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(tree, d_tree, tree_bytes, hipMemcpyDeviceToHost, pp.s_k)));
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(got, d_tree + tree_bytes - 32, 32, hipMemcpyDeviceToHost, pp.s_k)));
    }
    if (digests != nullptr)
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(digests, d_dig, n_rows * 32, hipMemcpyDeviceToHost, pp.s_k)));
    TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(pp.s_k)));
    if (root != nullptr) memcpy(root, got, 32);
    return call.finish(HADES252_OK);
}

// digests (may be NULL), tree (may be NULL) and root (NULL: no tree at all -- hades252_matrix_row_digests)
static int matrix_commit_host(const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride,
                              const uint64_t capacity_mont[4], int pad_mode, int arity, const uint64_t tag_mont[4], int out_idx,
                              const uint64_t *pad, uint64_t *digests, uint64_t *tree, uint64_t *root) {
    const bool with_tree = root != nullptr;
    const int depth = with_tree ? hades252_merkle_depth(n_rows, arity) : 0;
    int rc = check_device();
    if (rc != HADES252_OK) return rc;
    const size_t K = matrix_tile_rows(n_cols, n_rows);
    const size_t buf_b = up256(K * n_cols * 32), dig_b = up256(n_rows * 32);
    const size_t tree_b = up256(with_tree ? hades252_merkle_tree_bytes(n_rows, arity) : 0), pad_b = up256((size_t)depth * 32);
    HostCall call;
    rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    rc = pipe_ensure_aux(pp, 2 * buf_b + dig_b + tree_b + pad_b);
    if (rc != HADES252_OK) return call.finish(rc);
    uint8_t *d_buf = (uint8_t *)pp.aux, *d_dig = d_buf + 2 * buf_b, *d_tree = d_dig + dig_b, *d_pad = d_tree + tree_b;
    if (with_tree && pad != nullptr)                                   // the table is uploaded once, in front of everything
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_pad, pad, (size_t)depth * 32, hipMemcpyHostToDevice, pp.s_k)));
    rc = matrix_hash_rows(call, d_buf, K, planes, n_rows, n_cols, plane_stride, capacity_mont, pad_mode, d_dig);
    if (rc != HADES252_OK) return rc;                                  // (the call is finished already)
    return matrix_finish(call, d_dig, n_rows, arity, tag_mont, out_idx, pad != nullptr ? d_pad : nullptr, d_tree, digests, tree, root);
}

// the rules of a commitment's arguments, wherever its rows come from
static bool matrix_commit_args_ok(size_t n_rows, int pad_mode, int arity, const uint64_t *tag_mont, int out_idx,
                                  const uint64_t *pad, const uint64_t *digests, const uint64_t *tree, const uint64_t *root) {
    return hades252_merkle_depth(n_rows, arity) >= 1 && (pad_mode == 0 || pad_mode == 1) && tag_mont != nullptr &&
           root != nullptr && out_idx >= 0 && out_idx < 5 && !host_misaligned(pad) && !host_misaligned(digests) &&
           !host_misaligned(tree) && !host_misaligned(root);
}

int hades252_matrix_row_digests(const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride,
                                const uint64_t capacity_mont[4], int pad_mode, uint64_t *digests) {
    if (n_rows == 0) return HADES252_OK;
    if (!matrix_shape_ok(planes, n_rows, n_cols, plane_stride) || capacity_mont == nullptr || digests == nullptr ||
        host_misaligned(digests) || (pad_mode != 0 && pad_mode != 1))
        return HADES252_ERR_INVALID_ARG;
    return matrix_commit_host(planes, n_rows, n_cols, plane_stride, capacity_mont, pad_mode, 0, nullptr, 0, nullptr, digests,
                              nullptr, nullptr);
}

int hades252_matrix_commit(const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride,
                           const uint64_t capacity_mont[4], int pad_mode, int arity, const uint64_t tag_mont[4], int out_idx,
                           const uint64_t *pad, uint64_t *digests, uint64_t *tree, uint64_t root[4]) {
    if (!matrix_commit_args_ok(n_rows, pad_mode, arity, tag_mont, out_idx, pad, digests, tree, root) ||
        !matrix_shape_ok(planes, n_rows, n_cols, plane_stride) || capacity_mont == nullptr)
        return HADES252_ERR_INVALID_ARG;
    return matrix_commit_host(planes, n_rows, n_cols, plane_stride, capacity_mont, pad_mode, arity, tag_mont, out_idx, pad,
                              digests, tree, root);
}

// Openings from what hades252_matrix_commit returned: a gather in plain C++, no device.  Row r of the matrix, row-major,
// and its path in the layout of hades252_merkle_open_pad_dev: level 0 siblings are row digests, level l >= 1 siblings come
// from level l - 1 of `tree`, a sibling position past the end of its level is pad[l] (NULL: zero).
int hades252_matrix_open(const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride, const uint64_t *digests,
                         const uint64_t *tree, int arity, const uint64_t *pad, const uint64_t *indices, size_t n_queries,
                         uint64_t *rows_out, uint64_t *paths_out) {
    if (n_queries == 0) return HADES252_OK;
    const int depth = hades252_merkle_depth(n_rows, arity);
    if (depth < 1 || !matrix_shape_ok(planes, n_rows, n_cols, plane_stride) || digests == nullptr || tree == nullptr ||
        indices == nullptr || rows_out == nullptr || paths_out == nullptr || host_misaligned(digests) || host_misaligned(tree) ||
        host_misaligned(pad) || host_misaligned(indices) || host_misaligned(rows_out) || host_misaligned(paths_out) ||
        n_queries > SIZE_MAX / 32 / n_cols || n_queries > SIZE_MAX / 32 / ((size_t)depth * (arity - 1)))
        return HADES252_ERR_INVALID_ARG;
    const size_t path_words = (size_t)depth * (arity - 1) * 4;
    for (size_t t = 0; t < n_queries; t++) {
        uint64_t *row = rows_out + t * n_cols * 4, *path = paths_out + t * path_words;
        size_t node = (size_t)indices[t];
        if (indices[t] >= n_rows) {                                    // nothing outside the matrix or the tree is read
            memset(row, 0, n_cols * 32);
            memset(path, 0, path_words * 8);
            continue;
        }
        for (size_t c = 0; c < n_cols; c++) memcpy(row + c * 4, planes + (c * plane_stride + node) * 4, 32);
        const uint64_t *level = digests;
        size_t level_n = n_rows;
        for (int l = 0; l < depth; l++) {
            const size_t first = node - node % arity, pos = node % arity;
            for (int s = 0; s + 1 < arity; s++, path += 4) {
                const size_t sib = first + ((size_t)s < pos ? s : s + 1);
                if (sib < level_n)
                    memcpy(path, level + sib * 4, 32);
                else if (pad != nullptr)
                    memcpy(path, pad + (size_t)l * 4, 32);
                else
                    memset(path, 0, 32);
            }
            level = l == 0 ? tree : level + level_n * 4;
            level_n = (level_n + arity - 1) / arity;
            node /= arity;
        }
    }
    return HADES252_OK;
}

// roots[t] = the root recomputed from opened row t: the row-major sponge over the rows (hades252_sponge_hash_dev), then
// hades252_merkle_verify_dev on the digests -- both pick their latency forms for small batches of queries.
int hades252_matrix_verify(const uint64_t *rows, size_t n_cols, const uint64_t *indices, const uint64_t *paths, size_t n_queries,
                           int depth, int arity, const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                           int out_idx, uint64_t *roots) {
    if (n_queries == 0) return HADES252_OK;
    if (rows == nullptr || indices == nullptr || paths == nullptr || roots == nullptr || capacity_mont == nullptr ||
        tag_mont == nullptr || host_misaligned(rows) || host_misaligned(indices) || host_misaligned(paths) ||
        host_misaligned(roots) || n_cols < 1 || n_cols > HADES252_MATRIX_MAX_COLS || (pad_mode != 0 && pad_mode != 1) ||
        arity < 2 || arity > 4 || out_idx < 0 || out_idx >= 5 || depth < 1 || depth > 64 || n_queries > kMaxLaunchRecords ||
        n_queries > SIZE_MAX / 32 / n_cols || n_queries > SIZE_MAX / 32 / ((size_t)depth * (arity - 1)))
        return HADES252_ERR_INVALID_ARG;
    int rc = check_device();
    if (rc != HADES252_OK) return rc;
    const size_t rows_bytes = n_queries * n_cols * 32, idx_bytes = n_queries * 8;
    const size_t path_bytes = n_queries * (size_t)depth * (arity - 1) * 32, dig_b = up256(n_queries * 32);
    HostCall call;
    rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    rc = pipe_ensure_aux(pp, up256(rows_bytes) + up256(idx_bytes) + up256(path_bytes) + 2 * dig_b);
    if (rc != HADES252_OK) return call.finish(rc);
    uint8_t *d_rows = (uint8_t *)pp.aux, *d_idx = d_rows + up256(rows_bytes), *d_paths = d_idx + up256(idx_bytes);
    uint8_t *d_leaves = d_paths + up256(path_bytes), *d_roots = d_leaves + dig_b;
    TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_rows, rows, rows_bytes, hipMemcpyHostToDevice, pp.s_k)));
    TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_idx, indices, idx_bytes, hipMemcpyHostToDevice, pp.s_k)));
    TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_paths, paths, path_bytes, hipMemcpyHostToDevice, pp.s_k)));
    rc = hades252_sponge_hash_dev(d_rows, n_queries, n_cols, capacity_mont, pad_mode, d_leaves, pp.s_k);
    if (rc == HADES252_OK)
        rc = hades252_merkle_verify_dev(d_leaves, (const uint64_t *)d_idx, d_paths, n_queries, depth, arity, tag_mont, out_idx,
                                        d_roots, pp.s_k);
    if (rc != HADES252_OK) return call.finish(rc);
    TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(roots, d_roots, n_queries * 32, hipMemcpyDeviceToHost, pp.s_k)));
    TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(pp.s_k)));
    return call.finish(HADES252_OK);
}

}  // extern "C"
