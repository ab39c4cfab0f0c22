// host_matrix_stream.hpp -- C ABI, HOST memory in and out: streaming commitments to a matrix stored column by column
// (kernels_matrix_stream.hpp).  A commitment is opened for n_rows rows, fed any number of columns per call and finished at any
// point; the row sponges stay on the device in between, so the matrix never has to be in host memory at once, and a wide
// group runs as full-device launches of a few blocks each instead of thin launches of hundreds of blocks.
#pragma once

extern "C" {

// What an open stream holds.  The state planes (160 bytes per row) and, from the first finish on, the digests and the tree
// are the stream's own device memory, not the pool's: hades252_trim does not free them.  Streams, events and the two tile
// buffers are borrowed from the pool for the duration of a call.
struct MatrixStreamHandle {
    int device = -1;
    size_t n_rows = 0;
    uint64_t n_cols = 0;              // columns absorbed so far (the last good total)
    uint8_t *d_state = nullptr;       // five planes of n_rows words
    uint8_t *d_dig = nullptr;         // n_rows digests
    uint8_t *d_tree = nullptr;        // the tree, then the padding table
    size_t tree_cap = 0;
    bool poisoned = false;            // a HIP failure inside a call: nothing but cols and close works any more
};

// Columns per tile.  Test hook: HADES252_TEST_MATRIX_CHUNK_COLS (read once, at the first call; any value >= 1) sets it in
// place of the measured figure (it is rounded like that figure: 5 .. 7 mean 4), so that a group of a few columns runs through
// several tiles, with and without partial blocks (tests/test_gpu_f13_matrix_stream.py).
static size_t mstream_forced_cols() {
    static const size_t forced = []() -> size_t {
        const char *e = getenv("HADES252_TEST_MATRIX_CHUNK_COLS");
        return e ? (size_t)strtoull(e, nullptr, 0) : 0;
    }();
    return forced;
}

// what every call that touches the device asks first, once its arguments are good: not poisoned, on the stream's device
static int mstream_enter(const MatrixStreamHandle *h) {
    if (h->poisoned) return HADES252_ERR_HIP;
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    return dev == h->device ? HADES252_OK : HADES252_ERR_INVALID_ARG;
}

// The group in tiles of K rows x G columns, the measured constants of host_matrix.hpp: K = all rows up to kMatrixFullRows
// (a full device), G = kMatrixTargetBytes / (32 K) columns, a multiple of four where that leaves at least four -- the first
// tile is then shortened by the columns of the open block, so that only the first and the last tile of a call carry a
// partial block.  The tiles run through the two-buffer pipeline of host_matrix.hpp (matrix_tile_in, matrix_tile_launched); all
// kernels are ordered on the kernel stream and the column tiles are the outer loop, so every row sees its columns in order.
static int mstream_absorb_tiles(MatrixStreamHandle *ms, const uint64_t *planes, size_t n_cols, size_t plane_stride) {
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
    size_t t = 0;
    unsigned cur = (unsigned)(ms->n_cols % 4);
    for (size_t j = 0; j < n_cols;) {
        size_t gw = j == 0 && align ? G - cur : G;
        if (gw > n_cols - j) gw = n_cols - j;
        for (size_t off = 0; off < S; off += K, t++) {
            const size_t m = S - off < K ? S - off : K;
            uint8_t *d = (uint8_t *)pp.aux + t % 2 * buf_b;
            rc = matrix_tile_in(call, t, d, K, planes + (j * plane_stride + off) * 4, plane_stride, m, gw);
            if (rc != HADES252_OK) return rc;
            hipLaunchKernelGGL(k_planes_absorb, dim3(blocks_for(m)), dim3(kBlock), 0, pp.s_k, ms->d_state + off * 32, S, m, d, gw, K, (int)cur);
            rc = matrix_tile_launched(call, t);
            if (rc != HADES252_OK) return rc;
        }
        j += gw;
        cur = (unsigned)((cur + gw) % 4);
    }
    TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(pp.s_k)));           // the caller may reuse `planes`
    return call.finish(HADES252_OK);
}

// digests (may be NULL), tree (may be NULL) and root (NULL: no tree at all -- hades252_matstream_digests)
static int mstream_finish(MatrixStreamHandle *ms, int pad_mode, int arity, const uint64_t tag_mont[4], int out_idx,
                          const uint64_t *pad, uint64_t *digests, uint64_t *tree, uint64_t *root) {
    const size_t S = ms->n_rows;
    const bool with_tree = root != nullptr;
    const int depth = with_tree ? hades252_merkle_depth(S, arity) : 0;
    const size_t tree_b = up256(with_tree ? hades252_merkle_tree_bytes(S, arity) : 0), pad_b = up256((size_t)depth * 32);
    if (ms->d_dig == nullptr) HIP_TRY(F(F_MALLOC, hipMalloc((void **)&ms->d_dig, up256(S * 32))));
    if (with_tree && ms->tree_cap < tree_b + pad_b) {
        if (ms->d_tree) (void)hipFree(ms->d_tree);
        ms->d_tree = nullptr;
        ms->tree_cap = 0;
        HIP_TRY(F(F_MALLOC, hipMalloc((void **)&ms->d_tree, tree_b + pad_b)));
        ms->tree_cap = tree_b + pad_b;
    }
    uint8_t *d_pad = with_tree ? ms->d_tree + tree_b : nullptr;
    HostCall call;
    int rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    if (with_tree && pad != nullptr)
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_pad, pad, (size_t)depth * 32, hipMemcpyHostToDevice, pp.s_k)));
    hipLaunchKernelGGL(k_planes_finish, dim3(blocks_for(S)), dim3(kBlock), 0, pp.s_k, ms->d_state, S, S, ms->d_dig, (int)(ms->n_cols % 4), pad_mode);
    TRY_CALL(call, hipGetLastError());
    return matrix_finish(call, ms->d_dig, S, arity, tag_mont, out_idx, pad != nullptr ? d_pad : nullptr, ms->d_tree, digests, tree, root);
}

// (a failure with HADES252_ERR_HIP leaves the state planes, or the streams they were written on, in an unknown condition)
static int mstream_poison_on_hip(MatrixStreamHandle *ms, int rc) {
    if (rc == HADES252_ERR_HIP) ms->poisoned = true;
    return rc;
}

int hades252_matstream_close(void *ms) {
    MatrixStreamHandle *h = (MatrixStreamHandle *)ms;
    if (h == nullptr) return HADES252_OK;
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->d_dig) (void)hipFree(h->d_dig);
    if (h->d_tree) (void)hipFree(h->d_tree);
    (void)hipGetLastError();
    delete h;
    return HADES252_OK;
}

int hades252_matstream_open(void **out, size_t n_rows, const uint64_t capacity_mont[4]) {
    if (out == nullptr) return HADES252_ERR_INVALID_ARG;
    *out = nullptr;
    if (capacity_mont == nullptr || n_rows == 0 || n_rows > kMaxLaunchRecords) return HADES252_ERR_INVALID_ARG;
    int rc = check_device();
    if (rc != HADES252_OK) return rc;
    MatrixStreamHandle *ms = new (std::nothrow) MatrixStreamHandle();
    if (ms == nullptr) {
        tl_last_hip_error = (int)hipErrorOutOfMemory;
        return HADES252_ERR_HIP;
    }
    ms->n_rows = n_rows;
    auto opened = [&]() -> int {
        HIP_TRY(hipGetDevice(&ms->device));
        HIP_TRY(F(F_MALLOC, hipMalloc((void **)&ms->d_state, n_rows * 160)));
        HostCall call;
        int r = call.acquire(16);
        if (r != HADES252_OK) return r;
        hipLaunchKernelGGL(k_planes_init, dim3(blocks_for(n_rows)), dim3(kBlock), 0, call.pipe.s_k, ms->d_state, n_rows, n_rows,
                           fr_from_u64(capacity_mont));
        TRY_CALL(call, hipGetLastError());
        TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(call.pipe.s_k)));
        return call.finish(HADES252_OK);
    };
    rc = opened();
    if (rc != HADES252_OK) {
        (void)hades252_matstream_close(ms);
        return rc;
    }
    *out = ms;
    return HADES252_OK;
}

int hades252_matstream_absorb(void *ms, const uint64_t *planes, size_t n_cols, size_t plane_stride) {
    MatrixStreamHandle *h = (MatrixStreamHandle *)ms;
    if (h == nullptr) return HADES252_ERR_INVALID_ARG;
    if (n_cols == 0) return h->poisoned ? HADES252_ERR_HIP : HADES252_OK;
    if (planes == nullptr || host_misaligned(planes) || plane_stride < h->n_rows || plane_stride > SIZE_MAX / 32 / n_cols ||
        (uint64_t)n_cols > UINT64_MAX - h->n_cols)
        return HADES252_ERR_INVALID_ARG;
    int rc = mstream_enter(h);
    if (rc != HADES252_OK) return rc;
    rc = mstream_poison_on_hip(h, mstream_absorb_tiles(h, planes, n_cols, plane_stride));
    if (rc == HADES252_OK) h->n_cols += n_cols;
    return rc;
}

int hades252_matstream_cols(const void *ms, uint64_t *n_cols_so_far) {
    if (ms == nullptr || n_cols_so_far == nullptr) return HADES252_ERR_INVALID_ARG;
    *n_cols_so_far = ((const MatrixStreamHandle *)ms)->n_cols;
    return HADES252_OK;
}

int hades252_matstream_digests(void *ms, int pad_mode, uint64_t *digests) {
    MatrixStreamHandle *h = (MatrixStreamHandle *)ms;
    if (h == nullptr || h->n_cols == 0 || (pad_mode != 0 && pad_mode != 1) || digests == nullptr || host_misaligned(digests))
        return HADES252_ERR_INVALID_ARG;
    const int rc = mstream_enter(h);
    if (rc != HADES252_OK) return rc;
    return mstream_poison_on_hip(h, mstream_finish(h, pad_mode, 0, nullptr, 0, nullptr, digests, nullptr, nullptr));
}

int hades252_matstream_commit(void *ms, int pad_mode, int arity, const uint64_t tag_mont[4], int out_idx, const uint64_t *pad,
                              uint64_t *digests, uint64_t *tree, uint64_t root[4]) {
    MatrixStreamHandle *h = (MatrixStreamHandle *)ms;
    if (h == nullptr || h->n_cols == 0 || !matrix_commit_args_ok(h->n_rows, pad_mode, arity, tag_mont, out_idx, pad, digests, tree, root))
        return HADES252_ERR_INVALID_ARG;
    const int rc = mstream_enter(h);
    if (rc != HADES252_OK) return rc;
    return mstream_poison_on_hip(h, mstream_finish(h, pad_mode, arity, tag_mont, out_idx, pad, digests, tree, root));
}

}  // extern "C"
