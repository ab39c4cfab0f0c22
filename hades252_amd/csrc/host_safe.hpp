// host_safe.hpp -- C ABI, HOST memory in and out: the batched duplex sponge (abi_safe.hpp) on arrays in host memory, chunk by
// chunk through a pooled pipe as host_cipher.hpp runs the cipher, so that device memory stays bounded whatever the batch size.
#pragma once

extern "C" {

int hades252_safe_hash(const uint64_t *in, size_t n_msgs, const uint32_t *calls, size_t n_calls, const uint64_t tag_mont[4],
                       uint64_t *out) {
    if (n_msgs == 0) return HADES252_OK;
    SafePlan plan;
    if (in == nullptr || out == nullptr || tag_mont == nullptr || !safe_pattern_plan(calls, n_calls, plan) ||
        n_msgs > SIZE_MAX / ((plan.n_in + plan.n_out) * 32))
        return HADES252_ERR_INVALID_ARG;                                  // (the last: byte offsets of the arrays fit size_t)
    int rc = check_device();
    if (rc != HADES252_OK) return rc;
    const Fr tag = fr_from_u64(tag_mont);
    size_t chunk = host_chunk_bytes() / ((plan.n_in + plan.n_out) * 32);  // sponges per chunk
    if (chunk == 0) chunk = 1;
    if (chunk > n_msgs) chunk = n_msgs;
    if (chunk > kMaxLaunchRecords) chunk = kMaxLaunchRecords;
    const size_t in_b = chunk * plan.n_in * 32, out_b = chunk * plan.n_out * 32;
    HostCall call;
    rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    rc = pipe_ensure_aux(pp, in_b + out_b + 16);
    if (rc != HADES252_OK) return call.finish(rc);
    uint8_t *d_in = (uint8_t *)pp.aux, *d_out = d_in + in_b;
    const hipStream_t s = pp.s_k;
    const uint8_t *h_in = (const uint8_t *)in;
    uint8_t *h_out = (uint8_t *)out;
    for (size_t off = 0; off < n_msgs; off += chunk) {
        const size_t c = n_msgs - off < chunk ? n_msgs - off : chunk;
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_in, h_in + off * plan.n_in * 32, c * plan.n_in * 32, hipMemcpyHostToDevice, s)));
        rc = safe_launch(d_in, d_out, nullptr, c, plan, 0, tag, s);
        if (rc != HADES252_OK) return call.finish(rc);
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(h_out + off * plan.n_out * 32, d_out, c * plan.n_out * 32, hipMemcpyDeviceToHost, s)));
    }
    TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(s)));
    return call.finish(HADES252_OK);
}

}  // extern "C"
