// host_mmcs.hpp -- C ABI, HOST memory in and out: mixed-height matrix commitments (kernels_mmcs.hpp).  Several column-major
// matrices of different heights under ONE tree: the tree sits over the tallest matrix's row digests and the row digests of
// each shorter matrix are hashed into the level whose size equals its height.  One root, one path per query, and one launch
// that verifies a whole batch of openings.  Every height is a stream of host_matrix_stream.hpp, fed through its tiles.
#pragma once

extern "C" {

// What a commitment holds: one resident row-sponge stream per height (160 bytes of state and 32 of digest per row, the
// stream's own device memory), in the order of first use, and from the first commit on the tree.  hades252_trim frees none
// of it.
struct MmcsHandle {
    int device = -1;
    uint64_t capacity[4] = {0, 0, 0, 0};
    int n_groups = 0;
    MatrixStreamHandle *groups[HADES252_MMCS_MAX_GROUPS] = {};
    uint8_t *d_tree = nullptr;
    size_t tree_cap = 0;
    int tree_arity = 0;               // the tree of the last good commit: its arity and its tallest height (0: none)
    size_t tree_rows = 0;
    bool poisoned = false;            // a HIP failure inside a call: nothing but cols and free works any more
};

// Queries per chunk of a verification.  Test hook: HADES252_TEST_MMCS_CHUNK_QUERIES (read once, at the first call; any
// value >= 1) sets it, so that a few hundred queries run through several chunks (tests/test_gpu_f14_mmcs.py).
static size_t mmcs_forced_queries() {
    static const size_t forced = []() -> size_t {
        const char *e = getenv("HADES252_TEST_MMCS_CHUNK_QUERIES");
        return e ? (size_t)strtoull(e, nullptr, 0) : 0;
    }();
    return forced;
}

// n = arity^d -> d (d >= 0), else -1; arity 2 .. 4
static int mmcs_log(uint64_t n, int arity) {
    if (arity < 2 || arity > 4 || n == 0) return -1;
    int d = 0;
    for (; n > 1; n /= (uint64_t)arity, d++)
        if (n % (uint64_t)arity) return -1;
    return d;
}

size_t hades252_mmcs_tree_bytes(size_t max_rows, int arity) {
    if (mmcs_log(max_rows, arity) < 1 || max_rows > kMaxLaunchRecords) return 0;
    size_t total = 0;
    for (size_t n = max_rows; n >= 1; n /= (size_t)arity) total += n;   // a^D + ... + a + 1 digests
    return total * 32;
}

static int mmcs_enter(const MmcsHandle *h) {
    if (h->poisoned) return HADES252_ERR_HIP;
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    return dev == h->device ? HADES252_OK : HADES252_ERR_INVALID_ARG;
}

static int mmcs_poison_on_hip(MmcsHandle *h, int rc) {
    if (rc == HADES252_ERR_HIP) h->poisoned = true;
    return rc;
}

static MatrixStreamHandle *mmcs_group(const MmcsHandle *h, size_t n_rows) {
    for (int g = 0; g < h->n_groups; g++)
        if (h->groups[g]->n_rows == n_rows) return h->groups[g];
    return nullptr;
}

int hades252_mmcs_free(void *mc) {
    MmcsHandle *h = (MmcsHandle *)mc;
    if (h == nullptr) return HADES252_OK;
    for (int g = 0; g < h->n_groups; g++) (void)hades252_matstream_close(h->groups[g]);
    if (h->d_tree) (void)hipFree(h->d_tree);
    (void)hipGetLastError();
    delete h;
    return HADES252_OK;
}

int hades252_mmcs_new(void **out, const uint64_t capacity_mont[4]) {
    if (out == nullptr) return HADES252_ERR_INVALID_ARG;
    *out = nullptr;
    if (capacity_mont == nullptr) return HADES252_ERR_INVALID_ARG;
    int rc = check_device();
    if (rc != HADES252_OK) return rc;
    MmcsHandle *h = new (std::nothrow) MmcsHandle();
    if (h == nullptr) {
        tl_last_hip_error = (int)hipErrorOutOfMemory;
        return HADES252_ERR_HIP;
    }
    memcpy(h->capacity, capacity_mont, 32);
    const hipError_t e = hipGetDevice(&h->device);
    if (e != hipSuccess) {
        tl_last_hip_error = (int)e;
        (void)hipGetLastError();
        delete h;
        return HADES252_ERR_HIP;
    }
    *out = h;
    return HADES252_OK;
}

// a new height: its stream (the state planes, initialised) and its digests
static int mmcs_add_group(MmcsHandle *h, size_t n_rows, MatrixStreamHandle **out) {
    void *made = nullptr;
    int rc = hades252_matstream_open(&made, n_rows, h->capacity);
    if (rc != HADES252_OK) return rc;
    MatrixStreamHandle *ms = (MatrixStreamHandle *)made;
    const hipError_t e = F(F_MALLOC, hipMalloc((void **)&ms->d_dig, up256(n_rows * 32)));
    if (e != hipSuccess) {
        tl_last_hip_error = (int)e;
        (void)hipGetLastError();
        (void)hades252_matstream_close(ms);
        return HADES252_ERR_HIP;
    }
    h->groups[h->n_groups++] = ms;
    *out = ms;
    return HADES252_OK;
}

int hades252_mmcs_absorb(void *mc, const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride) {
    MmcsHandle *h = (MmcsHandle *)mc;
    if (h == nullptr) return HADES252_ERR_INVALID_ARG;
    if (n_cols == 0) return h->poisoned ? HADES252_ERR_HIP : HADES252_OK;
    if (n_rows == 0 || n_rows > kMaxLaunchRecords || planes == nullptr || host_misaligned(planes) || plane_stride < n_rows ||
        plane_stride > SIZE_MAX / 32 / n_cols)
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
    rc = mmcs_poison_on_hip(h, mstream_absorb_tiles(ms, planes, n_cols, plane_stride));
    if (rc == HADES252_OK) ms->n_cols += n_cols;
    return rc;
}

int hades252_mmcs_cols(const void *mc, size_t n_rows, uint64_t *n_cols_so_far) {
    if (mc == nullptr || n_cols_so_far == nullptr) return HADES252_ERR_INVALID_ARG;
    const MatrixStreamHandle *ms = mmcs_group((const MmcsHandle *)mc, n_rows);
    *n_cols_so_far = ms != nullptr ? ms->n_cols : 0;
    return HADES252_OK;
}

// The tree of a checked shape: order[0 .. G) are the groups by falling height, d[i] the level of order[i] (height = arity^d).
// Row digests first (the tallest group's straight into the tree's first level), then level by level towards the root on the
// pipe's kernel stream: hades252_merkle_level_dev picks the kernel form by the level's size, k_mmcs_inject follows where a
// group sits, and the levels above the shortest group are one hades252_merkle_build_dev (the layouts match: its leaves are
// the level just written, its tree what follows).  The digests never visit the host.
static int mmcs_commit_run(MmcsHandle *h, const int *order, const int *d, int pad_mode, int arity, const uint64_t tag_mont[4],
                           const uint64_t inject_tag_mont[4], int out_idx, uint64_t *tree, uint64_t *root) {
    const int G = h->n_groups, D = d[0];
    const size_t h0 = h->groups[order[0]]->n_rows, tree_bytes = hades252_mmcs_tree_bytes(h0, arity);
    h->tree_rows = 0;                                                  // the tree is rewritten from here on
    if (h->tree_cap < tree_bytes) {
        if (h->d_tree) (void)hipFree(h->d_tree);
        h->d_tree = nullptr;
        h->tree_cap = 0;
        HIP_TRY(F(F_MALLOC, hipMalloc((void **)&h->d_tree, up256(tree_bytes))));
        h->tree_cap = tree_bytes;
    }
    HostCall call;
    int rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    for (int i = 0; i < G; i++) {
        const MatrixStreamHandle *ms = h->groups[order[i]];
        const size_t S = ms->n_rows;
        uint8_t *dig = i == 0 ? h->d_tree : ms->d_dig;
        hipLaunchKernelGGL(k_planes_finish, dim3(blocks_for(S)), dim3(kBlock), 0, pp.s_k, ms->d_state, S, S, dig, (int)(ms->n_cols % 4), pad_mode);
        TRY_CALL(call, hipGetLastError());
    }
    const Fr inject_tag = fr_from_u64(inject_tag_mont);
    uint8_t *children = h->d_tree;
    size_t n = h0;                                                     // nodes of the level `children`
    int next = 1;                                                      // the next group to inject
    for (int l = D - 1; l >= 0 && next < G; l--) {
        uint8_t *parents = children + n * 32;
        n /= (size_t)arity;
        rc = hades252_merkle_level_dev(children, parents, n, arity, tag_mont, out_idx, pp.s_k);
        if (rc != HADES252_OK) return call.finish(rc);
        if (d[next] == l) {
            hipLaunchKernelGGL(k_mmcs_inject, dim3(blocks_for(n)), dim3(kBlock), 0, pp.s_k, parents, h->groups[order[next]]->d_dig, n, inject_tag, out_idx);
            TRY_CALL(call, hipGetLastError());
            next++;
        }
        children = parents;
    }
    if (n > 1) {
        rc = hades252_merkle_build_dev(children, n, arity, tag_mont, out_idx, children + n * 32, pp.s_k);
        if (rc != HADES252_OK) return call.finish(rc);
    }
    uint64_t got[4];                                                   // the caller's root is written on success only
    if (tree != nullptr) TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(tree, h->d_tree, tree_bytes, hipMemcpyDeviceToHost, pp.s_k)));
    TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(got, h->d_tree + tree_bytes - 32, 32, hipMemcpyDeviceToHost, pp.s_k)));
    TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(pp.s_k)));
    memcpy(root, got, 32);
    h->tree_arity = arity;
    h->tree_rows = h0;
    return call.finish(HADES252_OK);
}

int hades252_mmcs_commit(void *mc, int pad_mode, int arity, const uint64_t tag_mont[4], const uint64_t inject_tag_mont[4],
                         int out_idx, uint64_t *tree, uint64_t root[4]) {
    MmcsHandle *h = (MmcsHandle *)mc;
    if (h == nullptr || (pad_mode != 0 && pad_mode != 1) || arity < 2 || arity > 4 || tag_mont == nullptr ||
        inject_tag_mont == nullptr || out_idx < 0 || out_idx >= 5 || root == nullptr || host_misaligned(tree) ||
        host_misaligned(root) || h->n_groups < 1)
        return HADES252_ERR_INVALID_ARG;
    int order[HADES252_MMCS_MAX_GROUPS], d[HADES252_MMCS_MAX_GROUPS];
    for (int g = 0; g < h->n_groups; g++) {                            // by falling height (the heights are distinct)
        int i = g;
        for (; i > 0 && h->groups[order[i - 1]]->n_rows < h->groups[g]->n_rows; i--) order[i] = order[i - 1];
        order[i] = g;
    }
    for (int i = 0; i < h->n_groups; i++) {
        d[i] = mmcs_log(h->groups[order[i]]->n_rows, arity);
        if (d[i] < 0) return HADES252_ERR_INVALID_ARG;
    }
    if (d[0] < 1) return HADES252_ERR_INVALID_ARG;
    const int rc = mmcs_enter(h);
    if (rc != HADES252_OK) return rc;
    return mmcs_poison_on_hip(h, mmcs_commit_run(h, order, d, pad_mode, arity, tag_mont, inject_tag_mont, out_idx, tree, root));
}

// The path of index i < max_rows from the tree hades252_mmcs_commit returned: a gather in plain C++, no device -- what
// hades252_merkle_open_dev writes for d_leaves = the tree's first level, d_tree = the rest.  An index >= max_rows gives zeros.
int hades252_mmcs_open(const uint64_t *tree, size_t max_rows, int arity, const uint64_t *indices, size_t n_queries,
                       uint64_t *paths_out) {
    if (n_queries == 0) return HADES252_OK;
    const int depth = max_rows <= kMaxLaunchRecords ? mmcs_log(max_rows, arity) : -1;
    if (depth < 1 || tree == nullptr || indices == nullptr || paths_out == nullptr || host_misaligned(tree) ||
        host_misaligned(indices) || host_misaligned(paths_out) || n_queries > SIZE_MAX / 32 / ((size_t)depth * (arity - 1)))
        return HADES252_ERR_INVALID_ARG;
    const size_t path_words = (size_t)depth * (arity - 1) * 4;
    for (size_t t = 0; t < n_queries; t++) {
        uint64_t *path = paths_out + t * path_words;
        if (indices[t] >= max_rows) {                                  // nothing outside the tree is read
            memset(path, 0, path_words * 8);
            continue;
        }
        size_t node = (size_t)indices[t], level_n = max_rows;
        const uint64_t *level = tree;
        for (int l = 0; l < depth; l++) {
            const size_t first = node - node % arity, pos = node % arity;
            for (int s = 0; s + 1 < arity; s++, path += 4) memcpy(path, level + (first + ((size_t)s < pos ? s : s + 1)) * 4, 32);
            level += level_n * 4;
            level_n /= (size_t)arity;
            node /= (size_t)arity;
        }
    }
    return HADES252_OK;
}

// One chunk's launch: lane q of the grid runs the whole chain of query q.
static void mmcs_launch_verify(int arity, hipStream_t s, const uint8_t *d_rows, const uint64_t *d_idx, const uint8_t *d_paths, size_t m,
                               const MmcsGroups &table, uint32_t n_groups, size_t row_cols, uint32_t depth, size_t n_perms,
                               int pad_mode, const Fr &cap, const Fr &tag, const Fr &inject_tag, int out_idx, uint8_t *d_roots) {
#define HADES_LAUNCH_MMCS_VERIFY(A)                                                                                        \
    hipLaunchKernelGGL(k_mmcs_verify<A>, dim3(blocks_for(m)), dim3(kBlock), 0, s, d_rows, d_idx, d_paths, m, table, n_groups, \
                       row_cols, depth, n_perms, pad_mode, cap, tag, inject_tag, out_idx, d_roots)
    switch (arity) {
        case 2: HADES_LAUNCH_MMCS_VERIFY(2); break;
        case 3: HADES_LAUNCH_MMCS_VERIFY(3); break;
        default: HADES_LAUNCH_MMCS_VERIFY(4); break;
    }
#undef HADES_LAUNCH_MMCS_VERIFY
}

// The shape of a batch of openings as both verification calls check it (n_groups is 1 .. 32 and arity 2 .. 4 already):
// strictly falling powers of the arity from heights[0] >= arity, 1 .. 2^30 columns each, byte counts inside size_t.  -> the
// group table of k_mmcs_verify, the columns of a query's row, the permutations of a chain, the depth and a path's bytes.
struct MmcsShape {
    MmcsGroups table = {};
    size_t row_cols = 0, n_perms = 0, path_q = 0;
    int depth = 0;
};

static bool mmcs_verify_shape(const uint64_t *heights, const uint64_t *cols, size_t n_groups, int arity, int pad_mode,
                              size_t n_queries, MmcsShape &sh) {
    int prev = -1;
    for (size_t g = 0; g < n_groups; g++) {
        const int d = mmcs_log(heights[g], arity);
        if (d < 0 || (g == 0 ? d < 1 : d >= prev) || cols[g] < 1 || cols[g] > kMaxLaunchRecords) return false;
        if (g > 0) sh.table.climb[g - 1] = (uint32_t)(prev - d);
        sh.table.cols[g] = (uint32_t)cols[g];
        sh.row_cols += (size_t)cols[g];
        sh.n_perms += hades252_sponge_blocks((size_t)cols[g], pad_mode);
        prev = d;
    }
    sh.table.climb[n_groups - 1] = (uint32_t)prev;
    sh.depth = mmcs_log(heights[0], arity);
    sh.n_perms += (size_t)sh.depth + (n_groups - 1);                   // S = sum of blocks_g + D + (G - 1)
    sh.path_q = (size_t)sh.depth * (arity - 1) * 32;
    return n_queries <= SIZE_MAX / 32 / sh.row_cols && n_queries <= SIZE_MAX / sh.path_q;
}

// roots[t] = the root recomputed from opening t.  The queries travel in chunks of at most 2^18 queries and
// kMatrixTargetBytes of rows plus paths through the pooled pipe's two buffers: chunk i + 1 is copied on the copy stream
// while chunk i runs on the kernel stream, which also carries its roots back; the host runs at most two chunks ahead.
int hades252_mmcs_verify(const uint64_t *rows, const uint64_t *heights, const uint64_t *cols, size_t n_groups,
                         const uint64_t *indices, const uint64_t *paths, size_t n_queries, int arity,
                         const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                         const uint64_t inject_tag_mont[4], int out_idx, uint64_t *roots) {
    if (n_queries == 0) return HADES252_OK;
    if (rows == nullptr || heights == nullptr || cols == nullptr || indices == nullptr || paths == nullptr || roots == nullptr ||
        capacity_mont == nullptr || tag_mont == nullptr || inject_tag_mont == nullptr || host_misaligned(rows) ||
        host_misaligned(heights) || host_misaligned(cols) || host_misaligned(indices) || host_misaligned(paths) ||
        host_misaligned(roots) || n_groups < 1 || n_groups > HADES252_MMCS_MAX_GROUPS || arity < 2 || arity > 4 ||
        (pad_mode != 0 && pad_mode != 1) || out_idx < 0 || out_idx >= 5 || n_queries > kMaxLaunchRecords)
        return HADES252_ERR_INVALID_ARG;
    MmcsShape sh;
    if (!mmcs_verify_shape(heights, cols, n_groups, arity, pad_mode, n_queries, sh)) return HADES252_ERR_INVALID_ARG;
    const MmcsGroups &table = sh.table;
    const size_t row_cols = sh.row_cols, n_perms = sh.n_perms, path_q = sh.path_q;
    const int depth = sh.depth;
    int rc = check_device();
    if (rc != HADES252_OK) return rc;
    size_t M = mmcs_forced_queries();
    if (M == 0) {
        M = kMatrixTargetBytes / (row_cols * 32 + path_q);
        if (M > ((size_t)1 << 18)) M = (size_t)1 << 18;
    }
    if (M < 1) M = 1;
    if (M > n_queries) M = n_queries;
    const size_t rows_b = up256(M * row_cols * 32), idx_b = up256(M * 8), paths_b = up256(M * path_q), roots_b = up256(M * 32);
    const size_t buf_b = rows_b + idx_b + paths_b + roots_b;
    HostCall call;
    rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    rc = pipe_ensure_aux(pp, 2 * buf_b);
    if (rc != HADES252_OK) return call.finish(rc);
    const Fr cap = fr_from_u64(capacity_mont), tag = fr_from_u64(tag_mont), inject_tag = fr_from_u64(inject_tag_mont);
    size_t t = 0;
    for (size_t off = 0; off < n_queries; off += M, t++) {
        const size_t m = n_queries - off < M ? n_queries - off : M;
        const int k = (int)(t % 2);
        uint8_t *d_rows = (uint8_t *)pp.aux + (size_t)k * buf_b, *d_idx = d_rows + rows_b, *d_paths = d_idx + idx_b;
        uint8_t *d_roots = d_paths + paths_b;
        if (t >= 2) TRY_CALL(call, F(F_SYNC, hipEventSynchronize(pp.k_done[k])));      // chunk t - 2 is done: buffer k is free
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_rows, rows + off * row_cols * 4, m * row_cols * 32, hipMemcpyHostToDevice, pp.s_in)));
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_idx, indices + off, m * 8, hipMemcpyHostToDevice, pp.s_in)));
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_paths, (const uint8_t *)paths + off * path_q, m * path_q, hipMemcpyHostToDevice, pp.s_in)));
        TRY_CALL(call, hipEventRecord(pp.in_done[k], pp.s_in));
        TRY_CALL(call, hipStreamWaitEvent(pp.s_k, pp.in_done[k], 0));
        mmcs_launch_verify(arity, pp.s_k, d_rows, (const uint64_t *)d_idx, d_paths, m, table, (uint32_t)n_groups, row_cols, (uint32_t)depth,
                           n_perms, pad_mode, cap, tag, inject_tag, out_idx, d_roots);
        TRY_CALL(call, hipGetLastError());
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(roots + off * 4, d_roots, m * 32, hipMemcpyDeviceToHost, pp.s_k)));
        TRY_CALL(call, hipEventRecord(pp.k_done[k], pp.s_k));
    }
    TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(pp.s_k)));
    return call.finish(HADES252_OK);
}

}  // extern "C"
