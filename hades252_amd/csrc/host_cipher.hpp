// host_cipher.hpp -- C ABI, HOST memory in and out: the batched Poseidon cipher (abi_cipher.hpp) on arrays in host memory,
// chunk by chunk through a pooled pipe, so that device memory stays bounded whatever the batch size.
#pragma once

extern "C" {

// One stream (the pipe's kernel stream), one set of chunk buffers in the pipe's arena: upload keys, nonces and the chunk's
// messages / ciphers, run the cipher, download the result.  Simple and bounded; not pipelined (the cipher's throughput is
// that of the device entry points, where the data already lives on the device).
static int cipher_host(bool decrypt, const uint64_t *in, const uint64_t *keys, const uint64_t *nonces, size_t n, size_t len,
                       const uint64_t domain_mont[4], uint64_t *out, uint8_t *ok, size_t *n_rejected) {
    if (n_rejected != nullptr) *n_rejected = 0;
    if (n == 0) return HADES252_OK;
    if (in == nullptr || keys == nullptr || nonces == nullptr || out == nullptr || domain_mont == nullptr ||
        (decrypt && ok == nullptr) || len == 0 || len > HADES252_CIPHER_MAX_LEN || n > SIZE_MAX / ((len + 1) * 32))
        return HADES252_ERR_INVALID_ARG;                                  // (the last: byte offsets of the arrays fit size_t)
    int rc = check_device();
    if (rc != HADES252_OK) return rc;
    const size_t in_words = decrypt ? len + 1 : len, out_words = decrypt ? len : len + 1;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t per_msg = (in_words + out_words + 3) * 32 + 1;
    size_t chunk = host_chunk_bytes() / per_msg;                       // messages per chunk
    if (chunk == 0) chunk = 1;
    if (chunk > n) chunk = n;
    if (chunk > kMaxLaunchRecords) chunk = kMaxLaunchRecords;
    const size_t in_b = up16(chunk * in_words * 32), key_b = chunk * 64, nonce_b = chunk * 32,
                 out_b = up16(chunk * out_words * 32), ok_b = up16(chunk);
    HostCall call;
    rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    rc = pipe_ensure_aux(pp, in_b + key_b + nonce_b + out_b + ok_b + 16);
    if (rc != HADES252_OK) return call.finish(rc);
    uint8_t *d_in = (uint8_t *)pp.aux, *d_key = d_in + in_b, *d_nonce = d_key + key_b, *d_out = d_nonce + nonce_b;
    uint8_t *d_ok = d_out + out_b, *d_rej = d_ok + ok_b;
    const hipStream_t s = pp.s_k;
    // rejections: the device counter (an int) is cleared before every chunk and read back after it, and the chunks' counts
    // are summed in size_t here -- one chunk holds at most kMaxLaunchRecords < INT_MAX messages, the whole call any number
    std::vector<int> rej_chunk(decrypt ? (n + chunk - 1) / chunk : 0, 0);
    const uint8_t *h_in = (const uint8_t *)in, *h_key = (const uint8_t *)keys, *h_nonce = (const uint8_t *)nonces;
    uint8_t *h_out = (uint8_t *)out;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t c = n - off < chunk ? n - off : chunk;
        if (decrypt) TRY_CALL(call, hipMemsetAsync(d_rej, 0, 4, s));
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_in, h_in + off * in_words * 32, c * in_words * 32, hipMemcpyHostToDevice, s)));
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_key, h_key + off * 64, c * 64, hipMemcpyHostToDevice, s)));
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_nonce, h_nonce + off * 32, c * 32, hipMemcpyHostToDevice, s)));
        rc = cipher_launch(decrypt, d_in, d_key, d_nonce, c, len, domain_mont, d_out, decrypt ? d_ok : nullptr,
                           decrypt ? (int *)d_rej : nullptr, s);
        if (rc != HADES252_OK) return call.finish(rc);
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(h_out + off * out_words * 32, d_out, c * out_words * 32, hipMemcpyDeviceToHost, s)));
        if (decrypt) {
            TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(ok + off, d_ok, c, hipMemcpyDeviceToHost, s)));
            TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(&rej_chunk[off / chunk], d_rej, 4, hipMemcpyDeviceToHost, s)));
        }
    }
    TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(s)));
    size_t rejected = 0;
    for (int r : rej_chunk) rejected += (size_t)r;
    if (n_rejected != nullptr) *n_rejected = rejected;
    return call.finish(HADES252_OK);
}

int hades252_cipher_encrypt(const uint64_t *msgs, const uint64_t *keys, const uint64_t *nonces, size_t n_msgs, size_t msg_len,
                            const uint64_t domain_mont[4], uint64_t *ciphers) {
    return cipher_host(false, msgs, keys, nonces, n_msgs, msg_len, domain_mont, ciphers, nullptr, nullptr);
}

int hades252_cipher_decrypt(const uint64_t *ciphers, const uint64_t *keys, const uint64_t *nonces, size_t n_msgs,
                            size_t msg_len, const uint64_t domain_mont[4], uint64_t *msgs, uint8_t *ok, size_t *n_rejected) {
    return cipher_host(true, ciphers, keys, nonces, n_msgs, msg_len, domain_mont, msgs, ok, n_rejected);
}
#undef TRY_CALL

}  // extern "C"
