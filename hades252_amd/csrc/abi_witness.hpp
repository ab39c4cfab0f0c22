// abi_witness.hpp -- C ABI, device-resident data: gadget witnesses of the sponge (f1), of Merkle openings (f2) and of the
// cipher (f5), of the duplex sponge (f9), the permutation chains of row f4.  Every argument rule is checked before the
// device is touched;
// include/hades252.h holds the contracts.
#pragma once

extern "C" {

// permutations per message of hades252_sponge_hash_dev: ceil((msg_len + pad) / 4), at least one
size_t hades252_sponge_blocks(size_t msg_len, int pad_mode) {
    if (pad_mode != 0 && pad_mode != 1) return 0;
    const size_t b = msg_len / 4 + (msg_len % 4 + (size_t)pad_mode + 3) / 4;
    return b == 0 ? 1 : b;
}

int hades252_sponge_witness_dev(const void *d_msgs, size_t n_msgs, size_t msg_len, const uint64_t capacity_mont[4],
                                int pad_mode, void *d_inputs, void *d_wires, void *d_digests, void *stream) {
    if (n_msgs == 0) return HADES252_OK;
    if (capacity_mont == nullptr || (d_msgs == nullptr && msg_len > 0) || (pad_mode != 0 && pad_mode != 1) ||
        n_msgs > kMaxLaunchRecords || misaligned(d_msgs) || misaligned(d_digests) || d_inputs == nullptr ||
        d_wires == nullptr || misaligned(d_inputs) || misaligned(d_wires))
        return HADES252_ERR_INVALID_ARG;
    const size_t blocks = hades252_sponge_blocks(msg_len, pad_mode);
    if (blocks > kMaxLaunchRecords / n_msgs) return HADES252_ERR_INVALID_ARG;     // S * n_msgs records, at most 2^30
    if (pad_mode == 1)
        hipLaunchKernelGGL(k_witness_sponge<1>, dim3(blocks_for(n_msgs)), dim3(kBlock), 0, (hipStream_t)stream,
                           (const uint8_t *)d_msgs, n_msgs, msg_len, blocks, fr_from_u64(capacity_mont), (uint8_t *)d_inputs,
                           (uint8_t *)d_wires);
    else
        hipLaunchKernelGGL(k_witness_sponge<0>, dim3(blocks_for(n_msgs)), dim3(kBlock), 0, (hipStream_t)stream,
                           (const uint8_t *)d_msgs, n_msgs, msg_len, blocks, fr_from_u64(capacity_mont), (uint8_t *)d_inputs,
                           (uint8_t *)d_wires);
    HIP_TRY(hipGetLastError());
    if (d_digests != nullptr) {     // word 1 of the final states: r2[1] of the last round, records (S - 1) n .. S n - 1
        const size_t plane = blocks * n_msgs, first = (size_t)(kWitnessLastRow + 2) * plane + (blocks - 1) * n_msgs;
        HIP_TRY(hipMemcpyAsync(d_digests, (const uint8_t *)d_wires + first * 32, n_msgs * 32, hipMemcpyDeviceToDevice,
                               (hipStream_t)stream));
    }
    return HADES252_OK;
}

// The tree holds every node, so the depth x n_queries permutations of the openings are independent: one gather of their
// input states, then ONE k_perm_witness launch over all of them.
int hades252_merkle_open_witness_dev(const void *d_leaves, const void *d_tree, size_t n_leaves, int arity,
                                     const uint64_t tag_mont[4], const void *d_pad, const uint64_t *d_indices,
                                     size_t n_queries, void *d_inputs, void *d_wires, int *d_bad_count, void *stream) {
    const int depth = hades252_merkle_depth(n_leaves, arity);
    if (depth < 1) return HADES252_ERR_INVALID_ARG;
    if (n_queries == 0) return HADES252_OK;
    if (d_leaves == nullptr || d_tree == nullptr || d_indices == nullptr || tag_mont == nullptr || d_inputs == nullptr ||
        d_wires == nullptr || misaligned(d_leaves) || misaligned(d_tree) || misaligned(d_pad) || misaligned(d_inputs) ||
        misaligned(d_wires) || ((uintptr_t)d_bad_count & 3u) != 0)
        return HADES252_ERR_INVALID_ARG;
    if ((size_t)depth > kMaxLaunchRecords / n_queries) return HADES252_ERR_INVALID_ARG;
    const size_t n_perms = (size_t)depth * n_queries;
    hipStream_t s = (hipStream_t)stream;
    const Fr tag = fr_from_u64(tag_mont);
#define HADES_LAUNCH_PATH_STATES(A)                                                                                  \
    hipLaunchKernelGGL(k_witness_path_states<A>, dim3(blocks_for(n_perms * 5)), dim3(kBlock), 0, s,                  \
                       (const uint8_t *)d_leaves, (const uint8_t *)d_tree, n_leaves, depth, d_indices, n_queries, tag, \
                       (const uint8_t *)d_pad, (uint8_t *)d_inputs, d_bad_count)
    switch (arity) {
        case 2: HADES_LAUNCH_PATH_STATES(2); break;
        case 3: HADES_LAUNCH_PATH_STATES(3); break;
        default: HADES_LAUNCH_PATH_STATES(4); break;
    }
#undef HADES_LAUNCH_PATH_STATES
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_perm_witness, dim3(blocks_for(n_perms)), dim3(kBlock), 0, s, (const uint8_t *)d_inputs,
                       (uint8_t *)d_wires, n_perms);
    HIP_TRY(hipGetLastError());
    return HADES252_OK;
}

}  // extern "C"

// ---- gadget witnesses of the cipher (f5): k_witness_cipher, one message per lane ------------------------------------
// (after abi_cipher.hpp: its argument rules and fr_mont_of_u64 are reused)
extern "C" {

// permutations per message of hades252_cipher_*: ceil(M / 4) + 1 for a valid M, else 0
size_t hades252_cipher_perms(size_t msg_len) {
    if (msg_len == 0 || msg_len > HADES252_CIPHER_MAX_LEN) return 0;
    return (msg_len + 3) / 4 + 1;
}

}  // extern "C"

// the rules of hades252_cipher_*_dev (d_inputs in the place of their required output array) and of the chain witnesses;
// n > 0.  The side output `side` may be NULL.
static bool cipher_witness_args_bad(const void *in, const void *keys, const void *nonces, size_t n, size_t len,
                                    const uint64_t *domain_mont, const void *d_inputs, const void *d_wires, const void *side) {
    return cipher_args_bad(in, keys, nonces, n, len, domain_mont, d_inputs) || d_wires == nullptr || misaligned(d_wires) ||
           misaligned(side) || hades252_cipher_perms(len) > kMaxLaunchRecords / n;
}

// arguments already checked: n >= 1, S * n <= 2^30 (so n, M and S * n pass as 32-bit)
static int cipher_witness_launch(bool decrypt, const void *d_in, const void *d_keys, const void *d_nonces, size_t n,
                                 size_t len, const uint64_t domain_mont[4], void *d_inputs, void *d_wires, void *d_out,
                                 uint8_t *d_ok, int *d_rejected, hipStream_t s) {
    const Fr dom = fr_from_u64(domain_mont), lw = fr_mont_of_u64(len);
    const size_t steps = hades252_cipher_perms(len);
#define HADES_LAUNCH_CIPHER_WITNESS(D)                                                                                   \
    hipLaunchKernelGGL(k_witness_cipher<D>, dim3(blocks_for(n)), dim3(kBlock), 0, s, (const uint8_t *)d_in,              \
                       (const uint8_t *)d_keys, (const uint8_t *)d_nonces, (uint32_t)n, (uint32_t)len, (uint32_t)steps,   \
                       dom, lw, (uint8_t *)d_inputs,                                                                       \
                       (uint8_t *)d_wires, (uint8_t *)d_out, d_ok, d_rejected)
    if (decrypt)
        HADES_LAUNCH_CIPHER_WITNESS(true);
    else
        HADES_LAUNCH_CIPHER_WITNESS(false);
#undef HADES_LAUNCH_CIPHER_WITNESS
    HIP_TRY(hipGetLastError());
    return HADES252_OK;
}

extern "C" {

int hades252_cipher_encrypt_witness_dev(const void *d_msgs, const void *d_keys, const void *d_nonces, size_t n_msgs,
                                        size_t msg_len, const uint64_t domain_mont[4], void *d_inputs, void *d_wires,
                                        void *d_ciphers, void *stream) {
    if (n_msgs == 0) return HADES252_OK;
    if (cipher_witness_args_bad(d_msgs, d_keys, d_nonces, n_msgs, msg_len, domain_mont, d_inputs, d_wires, d_ciphers))
        return HADES252_ERR_INVALID_ARG;
    return cipher_witness_launch(false, d_msgs, d_keys, d_nonces, n_msgs, msg_len, domain_mont, d_inputs, d_wires, d_ciphers,
                                 nullptr, nullptr, (hipStream_t)stream);
}

int hades252_cipher_decrypt_witness_dev(const void *d_ciphers, const void *d_keys, const void *d_nonces, size_t n_msgs,
                                        size_t msg_len, const uint64_t domain_mont[4], void *d_inputs, void *d_wires,
                                        void *d_msgs, uint8_t *d_ok, int *d_rejected, void *stream) {
    if (n_msgs == 0) return HADES252_OK;
    if (cipher_witness_args_bad(d_ciphers, d_keys, d_nonces, n_msgs, msg_len, domain_mont, d_inputs, d_wires, d_msgs) ||
        misaligned4(d_rejected))
        return HADES252_ERR_INVALID_ARG;
    return cipher_witness_launch(true, d_ciphers, d_keys, d_nonces, n_msgs, msg_len, domain_mont, d_inputs, d_wires, d_msgs,
                                 d_ok, d_rejected, (hipStream_t)stream);
}

}  // extern "C"

// ---- gadget witnesses of the duplex sponge (f9): k_witness_duplex, one sponge per lane -------------------------------
// (after abi_safe.hpp: its planner, its cursor rule and its argument rules are reused).  There is no one-per-wave latency
// form, as for the other chain witnesses: every batch size runs per lane.

// arguments already checked: n >= 1, total_steps * n <= 2^30, step0 + plan.n_perms <= total_steps (so all pass as 32-bit).
// d_states == NULL: fresh sponges [tag, 0, 0, 0, 0] that end with the launch (plan.n_perms >= 1).
static int safe_witness_launch(const void *d_in, void *d_out, void *d_states, size_t n, const SafePlan &plan, uint32_t cursor,
                               const Fr &tag, void *d_inputs, void *d_wires, size_t step0, size_t total_steps, hipStream_t s) {
    hipLaunchKernelGGL(k_witness_duplex, dim3(blocks_for(n)), dim3(kBlock), 0, s, (const uint8_t *)d_in, (uint8_t *)d_out,
                       (uint8_t *)d_states, (uint32_t)n, (uint32_t)plan.n_in, (uint32_t)plan.n_out, plan.calls, plan.n_calls,
                       cursor, plan.n_perms, (uint32_t)step0, (uint32_t)total_steps, tag, (uint8_t *)d_inputs,
                       (uint8_t *)d_wires);
    HIP_TRY(hipGetLastError());
    return HADES252_OK;
}

// one streaming call with its records: the rules of safe_stream (abi_safe.hpp) and of the chain witnesses; *cursor and
// *step move on success only
static int safe_witness_stream(void *d_states, size_t n_states, const void *d_in, void *d_out, size_t len, uint32_t kind,
                               uint32_t *cursor, void *d_inputs, void *d_wires, size_t total_steps, size_t *step,
                               void *stream) {
    if (n_states == 0) return HADES252_OK;
    const void *d_words = kind ? d_in : d_out;
    if (d_states == nullptr || d_words == nullptr || cursor == nullptr || len == 0 || len > HADES252_SAFE_MAX_WORDS ||
        n_states > kMaxLaunchRecords || misaligned(d_states) || misaligned(d_words) || !safe_cursor_ok(*cursor))
        return HADES252_ERR_INVALID_ARG;
    if (d_inputs == nullptr || d_wires == nullptr || misaligned(d_inputs) || misaligned(d_wires) || step == nullptr ||
        total_steps > kMaxLaunchRecords / n_states || *step > total_steps)
        return HADES252_ERR_INVALID_ARG;
    const uint32_t call = kind | (uint32_t)len;
    SafePlan plan;
    if (!safe_plan(&call, 1, *cursor, plan) || plan.n_perms > total_steps - *step) return HADES252_ERR_INVALID_ARG;
    const int rc = safe_witness_launch(d_in, d_out, d_states, n_states, plan, *cursor, Fr{}, d_inputs, d_wires, *step,
                                       total_steps, (hipStream_t)stream);
    if (rc == HADES252_OK) {
        *cursor = plan.cursor_out;
        *step += plan.n_perms;
    }
    return rc;
}

extern "C" {

int hades252_safe_witness_dev(const void *d_in, size_t n_msgs, const uint32_t *calls, size_t n_calls,
                              const uint64_t tag_mont[4], void *d_inputs, void *d_wires, void *d_out, void *stream) {
    if (n_msgs == 0) return HADES252_OK;
    SafePlan plan;
    if (d_in == nullptr || tag_mont == nullptr || n_msgs > kMaxLaunchRecords || misaligned(d_in) || misaligned(d_out) ||
        d_inputs == nullptr || d_wires == nullptr || misaligned(d_inputs) || misaligned(d_wires) ||
        !safe_pattern_plan(calls, n_calls, plan))
        return HADES252_ERR_INVALID_ARG;
    if (plan.n_perms > kMaxLaunchRecords / n_msgs) return HADES252_ERR_INVALID_ARG;     // S * n_msgs records, at most 2^30
    return safe_witness_launch(d_in, d_out, nullptr, n_msgs, plan, 0, fr_from_u64(tag_mont), d_inputs, d_wires, 0,
                               plan.n_perms, (hipStream_t)stream);
}

int hades252_safe_absorb_witness_dev(void *d_states, size_t n_states, const void *d_in, size_t len, uint32_t *cursor,
                                     void *d_inputs, void *d_wires, size_t total_steps, size_t *step, void *stream) {
    return safe_witness_stream(d_states, n_states, d_in, nullptr, len, HADES252_SAFE_ABSORB, cursor, d_inputs, d_wires,
                               total_steps, step, stream);
}

int hades252_safe_squeeze_witness_dev(void *d_states, size_t n_states, size_t len, void *d_out, uint32_t *cursor,
                                      void *d_inputs, void *d_wires, size_t total_steps, size_t *step, void *stream) {
    return safe_witness_stream(d_states, n_states, nullptr, d_out, len, 0, cursor, d_inputs, d_wires, total_steps, step,
                               stream);
}

}  // extern "C"
