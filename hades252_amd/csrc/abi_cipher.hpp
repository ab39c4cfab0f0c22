// abi_cipher.hpp -- C ABI, device-resident data: the batched Poseidon cipher (kernels_cipher.hpp), encrypt and decrypt, routed
// by batch size as sponge_launch routes the sponge (one message per wave up to kLanesMaxStates, one per lane above).
#pragma once

// m * 2^256 mod p (the Montgomery form of the small integer m): 256 doublings mod p.  p < 2^255, so 2r never overflows.
static Fr fr_mont_of_u64(uint64_t m) {
    static const uint64_t P[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
    uint64_t r[4] = {m, 0, 0, 0};                    // m < p
    for (int it = 0; it < 256; it++) {
        uint64_t t[4];
        t[3] = (r[3] << 1) | (r[2] >> 63);
        t[2] = (r[2] << 1) | (r[1] >> 63);
        t[1] = (r[1] << 1) | (r[0] >> 63);
        t[0] = r[0] << 1;
        bool ge = true;                              // t >= p ?
        for (int k = 3; k >= 0; k--)
            if (t[k] != P[k]) {
                ge = t[k] > P[k];
                break;
            }
        if (ge) {
            unsigned __int128 borrow = 0;
            for (int k = 0; k < 4; k++) {
                const unsigned __int128 d = (unsigned __int128)t[k] - P[k] - borrow;
                t[k] = (uint64_t)d;
                borrow = (d >> 64) ? 1 : 0;
            }
        }
        for (int k = 0; k < 4; k++) r[k] = t[k];
    }
    return fr_from_u64(r);
}

// arguments already checked; n >= 1
static int cipher_launch(bool decrypt, const void *d_in, const void *d_keys, const void *d_nonces, size_t n, size_t len,
                         const uint64_t domain_mont[4], void *d_out, uint8_t *d_ok, int *d_rejected, hipStream_t s) {
    const Fr dom = fr_from_u64(domain_mont), lw = fr_mont_of_u64(len);
    const uint8_t *in = (const uint8_t *)d_in, *keys = (const uint8_t *)d_keys, *nonces = (const uint8_t *)d_nonces;
    uint8_t *out = (uint8_t *)d_out;
    if (n <= kLanesMaxStates) {                          // a few messages: one per wave
        const bool helped = n <= kLanesHelpedMaxStates;
        const unsigned per = helped ? kLanesWaves - 1 : kLanesWaves;
        const dim3 grid((unsigned)((n + per - 1) / per)), block(kLanesWaves * kWave);
#define HADES_LAUNCH_CIPHER_LANES(D, H) \
    hipLaunchKernelGGL((k_cipher_lanes<D, H>), grid, block, 0, s, in, keys, nonces, out, d_ok, d_rejected, n, len, dom, lw)
        if (decrypt && helped) HADES_LAUNCH_CIPHER_LANES(true, true);
        else if (decrypt) HADES_LAUNCH_CIPHER_LANES(true, false);
        else if (helped) HADES_LAUNCH_CIPHER_LANES(false, true);
        else HADES_LAUNCH_CIPHER_LANES(false, false);
#undef HADES_LAUNCH_CIPHER_LANES
    } else if (decrypt) {
        hipLaunchKernelGGL(k_cipher<true>, dim3(blocks_for(n)), dim3(kBlock), lds_for(4), s, in, keys, nonces, out, d_ok,
                           d_rejected, n, len, dom, lw);
    } else {
        hipLaunchKernelGGL(k_cipher<false>, dim3(blocks_for(n)), dim3(kBlock), lds_for(4), s, in, keys, nonces, out, d_ok,
                           d_rejected, n, len, dom, lw);
    }
    HIP_TRY(hipGetLastError());
    return HADES252_OK;
}

static bool misaligned4(const void *p) { return ((uintptr_t)p & 3u) != 0; }

// the argument rules of both directions (n > 0): every array present and 16-byte aligned (the counter: 4-byte), a length in
// 1 .. HADES252_CIPHER_MAX_LEN, at most kMaxLaunchRecords messages
static bool cipher_args_bad(const void *in, const void *keys, const void *nonces, size_t n, size_t len,
                            const uint64_t *domain_mont, const void *out) {
    return in == nullptr || keys == nullptr || nonces == nullptr || out == nullptr || domain_mont == nullptr || len == 0 ||
           len > HADES252_CIPHER_MAX_LEN || n > kMaxLaunchRecords || misaligned(in) || misaligned(keys) ||
           misaligned(nonces) || misaligned(out);
}

extern "C" {

int hades252_cipher_encrypt_dev(const void *d_msgs, const void *d_keys, const void *d_nonces, size_t n_msgs, size_t msg_len,
                                const uint64_t domain_mont[4], void *d_ciphers, void *stream) {
    if (n_msgs == 0) return HADES252_OK;
    if (cipher_args_bad(d_msgs, d_keys, d_nonces, n_msgs, msg_len, domain_mont, d_ciphers)) return HADES252_ERR_INVALID_ARG;
    return cipher_launch(false, d_msgs, d_keys, d_nonces, n_msgs, msg_len, domain_mont, d_ciphers, nullptr, nullptr,
                         (hipStream_t)stream);
}

int hades252_cipher_decrypt_dev(const void *d_ciphers, const void *d_keys, const void *d_nonces, size_t n_msgs,
                                size_t msg_len, const uint64_t domain_mont[4], void *d_msgs, uint8_t *d_ok, int *d_rejected,
                                void *stream) {
    if (n_msgs == 0) return HADES252_OK;
    if (cipher_args_bad(d_ciphers, d_keys, d_nonces, n_msgs, msg_len, domain_mont, d_msgs) || d_ok == nullptr ||
        misaligned4(d_rejected))
        return HADES252_ERR_INVALID_ARG;
    return cipher_launch(true, d_ciphers, d_keys, d_nonces, n_msgs, msg_len, domain_mont, d_msgs, d_ok, d_rejected,
                         (hipStream_t)stream);
}

}  // extern "C"
