// host_inverse.hpp -- C ABI, HOST memory in and out, in place: the inverse permutation, a range of its rounds, and batched
// fifth roots (kernels_inverse.hpp).  A state costs about 17 forward permutations of arithmetic for the same 160 bytes each
// way, so the copies hide behind the kernel and there is no device-pointer form.
#pragma once

extern "C" {

// Chunk by chunk through a pooled pipe: two chunk buffers in the pipe's arena, used alternately, and the pipe's three
// streams chained by its events -- chunk c + 1 travels to the device and chunk c - 1 back while chunk c is in the kernel,
// which is where the time goes.  Device memory is bounded by two chunks whatever n is.  rec_bytes: 160 (states) or 32
// (scalars).  The host runs at most two chunks ahead: it waits for the copy-out of the chunk that last used a buffer.
static int inverse_host(bool scalars, uint64_t *data, size_t n, int round_hi, int round_lo) {
    if (n == 0) return HADES252_OK;
    const size_t rec_bytes = scalars ? 32 : 160;
    if (data == nullptr || ((uintptr_t)data & 7u) != 0 || n > SIZE_MAX / rec_bytes || round_lo < 0 || round_lo > round_hi ||
        round_hi > HADES252_ROUNDS_TOTAL)
        return HADES252_ERR_INVALID_ARG;
    if (round_hi == round_lo) return HADES252_OK;
    int rc = check_device();
    if (rc != HADES252_OK) return rc;
    size_t chunk = host_chunk_bytes() / rec_bytes;                     // records per chunk
    if (chunk == 0) chunk = 1;
    if (chunk > n) chunk = n;
    if (chunk > kMaxLaunchRecords) chunk = kMaxLaunchRecords;
    const size_t buf_b = (chunk * rec_bytes + 255) & ~(size_t)255;
    HostCall call;
    rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    rc = pipe_ensure_aux(pp, 2 * buf_b);
    if (rc != HADES252_OK) return call.finish(rc);
    uint8_t *h = (uint8_t *)data;
    const size_t n_chunks = (n + chunk - 1) / chunk;
    for (size_t c = 0; c < n_chunks; c++) {
        const int k = (int)(c % 2);
        const size_t off = c * chunk, m = n - off < chunk ? n - off : chunk;
        uint8_t *d = (uint8_t *)pp.aux + (size_t)k * buf_b;
        if (c >= 2) TRY_CALL(call, F(F_SYNC, hipEventSynchronize(pp.out_done[k])));      // chunk c - 2 has left buffer k
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d, h + off * rec_bytes, m * rec_bytes, hipMemcpyHostToDevice, pp.s_in)));
        TRY_CALL(call, hipEventRecord(pp.in_done[k], pp.s_in));
        TRY_CALL(call, hipStreamWaitEvent(pp.s_k, pp.in_done[k], 0));
        if (scalars)
            hipLaunchKernelGGL(k_fifth_root, dim3(blocks_for(m)), dim3(kBlock), 0, pp.s_k, d, m);
        else
            hipLaunchKernelGGL(k_perm_inverse, dim3(blocks_for(m)), dim3(kBlock), lds_for(5), pp.s_k, d, m, round_hi, round_lo);
        TRY_CALL(call, hipGetLastError());
        TRY_CALL(call, hipEventRecord(pp.k_done[k], pp.s_k));
        TRY_CALL(call, hipStreamWaitEvent(pp.s_out, pp.k_done[k], 0));
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(h + off * rec_bytes, d, m * rec_bytes, hipMemcpyDeviceToHost, pp.s_out)));
        TRY_CALL(call, hipEventRecord(pp.out_done[k], pp.s_out));
    }
    TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(pp.s_out)));       // the last copy-out is behind everything else
    return call.finish(HADES252_OK);
}

int hades252_perm_inverse_batch(uint64_t *states, size_t n_perms) {
    return inverse_host(false, states, n_perms, HADES252_ROUNDS_TOTAL, 0);
}

int hades252_perm_inverse_rounds(uint64_t *states, size_t n_perms, int round_hi, int round_lo) {
    return inverse_host(false, states, n_perms, round_hi, round_lo);
}

int hades252_fifth_root_batch(uint64_t *scalars, size_t n_scalars) {
    return inverse_host(true, scalars, n_scalars, 1, 0);
}

}  // extern "C"
