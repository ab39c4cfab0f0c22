// abi_safe.hpp -- C ABI, device-resident data: the batched duplex sponge (kernels_safe.hpp), the whole IO pattern in one launch
// and the streaming absorb / squeeze calls, routed by batch size as cipher_launch routes the cipher (one sponge per wave up to
// kLanesMaxStates, one per lane above; 1 025 .. 16 384 sponges run per lane too, as the cipher's messages do).
#pragma once

// A sequence of calls, aggregated (consecutive calls of one kind are one call of the summed length), with what it moves and
// costs when it starts at `cursor` (pos_absorb | pos_squeeze << 4, 0 = a fresh sponge).
struct SafePlan {
    SafeCalls calls;
    uint32_t n_calls, n_perms, cursor_out;
    size_t n_in, n_out;
};

static bool safe_cursor_ok(uint32_t cursor) {
    const uint32_t pa = cursor & 15u, ps = cursor >> 4;
    return pa <= 4 && ps <= 4 && (pa == 0 || ps == 4);               // words were added: the next squeeze permutes first
}

// false: a call of length 0, more than HADES252_SAFE_MAX_CALLS calls, or more than HADES252_SAFE_MAX_WORDS words in or out.
// The permutation count is closed-form per aggregated call: a call of L words that starts at position q permutes
// floor((q + L - 1) / 4) times and ends at position (q + L - 1) mod 4 + 1.
static bool safe_plan(const uint32_t *calls, size_t n_calls, uint32_t cursor, SafePlan &plan) {
    if (calls == nullptr || n_calls == 0 || n_calls > HADES252_SAFE_MAX_CALLS) return false;
    plan.n_calls = 0;
    plan.n_in = plan.n_out = 0;
    for (size_t i = 0; i < n_calls; i++) {
        const uint32_t kind = calls[i] & HADES252_SAFE_ABSORB, len = calls[i] & ~HADES252_SAFE_ABSORB;
        if (len == 0 || len > HADES252_SAFE_MAX_WORDS) return false;
        size_t &total = kind ? plan.n_in : plan.n_out;
        total += len;
        if (total > HADES252_SAFE_MAX_WORDS) return false;
        if (plan.n_calls > 0 && (plan.calls.c[plan.n_calls - 1] & HADES252_SAFE_ABSORB) == kind)
            plan.calls.c[plan.n_calls - 1] += len;
        else
            plan.calls.c[plan.n_calls++] = kind | len;
    }
    for (uint32_t i = plan.n_calls; i < HADES252_SAFE_MAX_CALLS; i++) plan.calls.c[i] = 0;
    uint32_t pa = cursor & 15u, ps = cursor >> 4, perms = 0;
    for (uint32_t i = 0; i < plan.n_calls; i++) {
        const uint32_t len = plan.calls.c[i] & ~HADES252_SAFE_ABSORB;
        if (plan.calls.c[i] & HADES252_SAFE_ABSORB) {
            perms += (pa + len - 1) / 4;
            pa = (pa + len - 1) % 4 + 1;
            ps = 4;
        } else {
            const uint32_t q = (ps + len - 1) / 4;
            perms += q;
            ps = (ps + len - 1) % 4 + 1;
            if (q > 0) pa = 0;
        }
    }
    plan.n_perms = perms;
    plan.cursor_out = pa | (ps << 4);
    return true;
}

// a whole IO pattern: starts with an absorb, ends with a squeeze
static bool safe_pattern_plan(const uint32_t *calls, size_t n_calls, SafePlan &plan) {
    return safe_plan(calls, n_calls, 0, plan) && (calls[0] & HADES252_SAFE_ABSORB) != 0 &&
           (calls[n_calls - 1] & HADES252_SAFE_ABSORB) == 0;
}

// arguments already checked; n >= 1.  d_states == NULL: fresh sponges [tag, 0, 0, 0, 0] that end with the launch.
static int safe_launch(const void *d_in, void *d_out, void *d_states, size_t n, const SafePlan &plan, uint32_t cursor,
                       const Fr &tag, hipStream_t s) {
    const uint8_t *in = (const uint8_t *)d_in;
    uint8_t *out = (uint8_t *)d_out, *states = (uint8_t *)d_states;
    if (n <= kLanesMaxStates) {                          // a few sponges: one per wave
        const bool helped = n <= kLanesHelpedMaxStates;
        const unsigned per = helped ? kLanesWaves - 1 : kLanesWaves;
        const dim3 grid((unsigned)((n + per - 1) / per)), block(kLanesWaves * kWave);
        if (helped)
            hipLaunchKernelGGL(k_safe_lanes<true>, grid, block, 0, s, in, out, states, n, plan.n_in, plan.n_out, plan.calls,
                               plan.n_calls, cursor, plan.n_perms, tag);
        else
            hipLaunchKernelGGL(k_safe_lanes<false>, grid, block, 0, s, in, out, states, n, plan.n_in, plan.n_out, plan.calls,
                               plan.n_calls, cursor, plan.n_perms, tag);
    } else {
        hipLaunchKernelGGL(k_safe, dim3(blocks_for(n)), dim3(kBlock), lds_for(5), s, in, out, states, n, plan.n_in, plan.n_out,
                           plan.calls, plan.n_calls, cursor, plan.n_perms, tag);
    }
    HIP_TRY(hipGetLastError());
    return HADES252_OK;
}

extern "C" {

int hades252_safe_pattern(const uint32_t *calls, size_t n_calls, size_t *n_in, size_t *n_out, size_t *n_perms) {
    SafePlan plan;
    if (!safe_pattern_plan(calls, n_calls, plan)) return HADES252_ERR_INVALID_ARG;
    if (n_in != nullptr) *n_in = plan.n_in;
    if (n_out != nullptr) *n_out = plan.n_out;
    if (n_perms != nullptr) *n_perms = plan.n_perms;
    return HADES252_OK;
}

int hades252_safe_hash_dev(const void *d_in, size_t n_msgs, const uint32_t *calls, size_t n_calls, const uint64_t tag_mont[4],
                           void *d_out, void *stream) {
    if (n_msgs == 0) return HADES252_OK;
    SafePlan plan;
    if (d_in == nullptr || d_out == nullptr || tag_mont == nullptr || n_msgs > kMaxLaunchRecords || misaligned(d_in) ||
        misaligned(d_out) || !safe_pattern_plan(calls, n_calls, plan))
        return HADES252_ERR_INVALID_ARG;
    return safe_launch(d_in, d_out, nullptr, n_msgs, plan, 0, fr_from_u64(tag_mont), (hipStream_t)stream);
}

// one streaming call: `len` words of one kind for every state, from *cursor on; *cursor moves on success only
static int safe_stream(void *d_states, size_t n_states, const void *d_in, void *d_out, size_t len, uint32_t kind,
                       uint32_t *cursor, void *stream) {
    if (n_states == 0) return HADES252_OK;
    const void *d_words = kind ? d_in : d_out;
    if (d_states == nullptr || d_words == nullptr || cursor == nullptr || len == 0 || len > HADES252_SAFE_MAX_WORDS ||
        n_states > kMaxLaunchRecords || misaligned(d_states) || misaligned(d_words) || !safe_cursor_ok(*cursor))
        return HADES252_ERR_INVALID_ARG;
    const uint32_t call = kind | (uint32_t)len;
    SafePlan plan;
    if (!safe_plan(&call, 1, *cursor, plan)) return HADES252_ERR_INVALID_ARG;
    const int rc = safe_launch(d_in, d_out, d_states, n_states, plan, *cursor, Fr{}, (hipStream_t)stream);
    if (rc == HADES252_OK) *cursor = plan.cursor_out;
    return rc;
}

int hades252_safe_absorb_dev(void *d_states, size_t n_states, const void *d_in, size_t len, uint32_t *cursor, void *stream) {
    return safe_stream(d_states, n_states, d_in, nullptr, len, HADES252_SAFE_ABSORB, cursor, stream);
}

int hades252_safe_squeeze_dev(void *d_states, size_t n_states, size_t len, void *d_out, uint32_t *cursor, void *stream) {
    return safe_stream(d_states, n_states, nullptr, d_out, len, 0, cursor, stream);
}

}  // extern "C"
