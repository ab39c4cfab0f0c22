// kernels_safe.hpp -- batched duplex sponge (SAFE: an IO pattern of absorb / squeeze calls, no padding): one sponge per lane, one per wave
// Part of the single translation unit hades252.hip (included there after kernels_cipher.hpp); not a stand-alone header.
#pragma once

// The construction dusk-poseidon moved its hash, Merkle level and cipher onto after 0.33 (crate dusk-safe).  Neither crate is
// part of the reference tree: the construction below is recalled from them, the tag word is a call parameter and parity is
// pinned only to this repository's model (tests/safe_model.py): CONVENTION UNPINNED.  Rate 4, width 5:
//   state = [tag, 0, 0, 0, 0]; pos_absorb = 0; pos_squeeze = 0
//   absorb(x ..):  for each x: if pos_absorb == 4: perm, pos_absorb = 0;   state[1 + pos_absorb] += x, pos_absorb += 1
//                  afterwards pos_squeeze = 4                                 (the next squeeze permutes first)
//   squeeze(n):    n times: if pos_squeeze == 4: perm, pos_squeeze = 0, pos_absorb = 0;   emit state[1 + pos_squeeze], += 1
// Between two permutations a sponge therefore first emits j <= 4 words and then adds k <= 4 words: one SafeStep.  Every
// sponge of a launch follows the same calls, so the steps are wave-uniform scalar work derived from the (at most 64)
// aggregated calls in the kernel arguments: no per-step table, whatever the pattern's length.

struct SafeCalls {
    uint32_t c[HADES252_SAFE_MAX_CALLS];      // aggregated (kinds alternate): bit 31 = absorb, low 31 bits = length
};
// where a sponge stands: the call being served and what is left of it, the two positions (0 .. 4)
struct SafeWalk {
    uint32_t ci, rem, pa, ps;
};
// emit words at positions [e0, e0 + j), then add words at positions [a0, a0 + k)
struct SafeStep {
    int e0, j, a0, k;
};

__device__ __forceinline__ bool safe_is_absorb(const SafeCalls &calls, uint32_t ci) { return (calls.c[ci] >> 31) != 0; }

__device__ __forceinline__ SafeWalk safe_begin(const SafeCalls &calls, uint32_t cursor) {
    SafeWalk w;
    w.ci = 0;
    w.rem = calls.c[0] & 0x7fffffffu;
    w.pa = cursor & 15u;
    w.ps = cursor >> 4;
    return w;
}

// what happens before the next permutation (nothing, once the calls are used up)
__device__ __forceinline__ SafeStep safe_step(const SafeCalls &calls, uint32_t n_calls, SafeWalk &w) {
    SafeStep s = {(int)w.ps, 0, (int)w.pa, 0};
    if (w.ci < n_calls && !safe_is_absorb(calls, w.ci) && w.ps < 4) {
        const uint32_t room = 4 - w.ps;
        s.j = (int)(w.rem < room ? w.rem : room);
        w.rem -= s.j;
        w.ps += s.j;
        if (w.rem == 0 && ++w.ci < n_calls) w.rem = calls.c[w.ci] & 0x7fffffffu;
    }
    if (w.ci < n_calls && safe_is_absorb(calls, w.ci) && w.pa < 4) {
        const uint32_t room = 4 - w.pa;
        s.k = (int)(w.rem < room ? w.rem : room);
        w.rem -= s.k;
        w.pa += s.k;
        w.ps = 4;
        if (w.rem == 0 && ++w.ci < n_calls) w.rem = calls.c[w.ci] & 0x7fffffffu;
    }
    return s;
}

// the permutation an unfinished call asked for has run
__device__ __forceinline__ void safe_permuted(const SafeCalls &calls, uint32_t n_calls, SafeWalk &w) {
    w.pa = 0;
    if (w.ci < n_calls && !safe_is_absorb(calls, w.ci)) w.ps = 0;
}

// ---- one sponge per lane (throughput) -----------------------------------------------------------------------------
// in: n x n_in words, out: n x n_out words (AoS, message-major), moved through the wave's LDS slab with the cipher's
// gather / scatter (8 lanes per message, 16 bytes each).  n_perms permutations through ONE call site; the host counts
// them (abi_safe.hpp) and every wave runs exactly that many, so the trip count never depends on the walk.
// states != NULL (streaming): the 160-byte states are loaded at the start and stored at the end, `cursor` holds the
// positions the previous call left; states == NULL: a fresh sponge [tag, 0, 0, 0, 0] that ends with the launch.
__global__ void __launch_bounds__(kBlock, 3) k_safe(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint8_t *states,
                                                    size_t n, size_t n_in, size_t n_out, SafeCalls calls, uint32_t n_calls,
                                                    uint32_t cursor, uint32_t n_perms, Fr tag) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *slab = wave_slab<5>(lds);                               // 5-word records for the states, 4-word ones inside it
    const size_t rec0 = (size_t)blockIdx.x * kBlock + (threadIdx.x / kWave) * kWave;
    Fr st[5];
    if (states != nullptr) {
        wave_load_records<5>(states, rec0, n, slab, st);             // (block-wide barriers: uniform across the block)
    } else {
        st[0] = tag;
#pragma unroll
        for (int w = 1; w < 5; w++) st[w] = zero_word();
    }
    SafeWalk walk = safe_begin(calls, cursor);
    size_t in_off = 0, out_off = 0;
#pragma unroll 1
    for (uint32_t t = 0;; t++) {
        const SafeStep s = safe_step(calls, n_calls, walk);
        if (s.j > 0) {
            const Fr o4[4] = {st[1], st[2], st[3], st[4]};
            cipher_scatter<false>(out, n_out, out_off, s.j, rec0, n, slab, o4, false, s.e0);
            out_off += s.j;
        }
        if (s.k > 0) {
            Fr w4[4];
            cipher_gather(in, n_in, in_off, s.k, rec0, n, slab, w4, s.a0);
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i >= s.a0 && i < s.a0 + s.k) st[1 + i] = fr_add(st[1 + i], w4[i]);
            in_off += s.k;
        }
        if (t == n_perms) break;
        Fr out5[5];
        fast_perm<5>(&d_fast, st, out5, 0);
#pragma unroll
        for (int w = 0; w < 5; w++) st[w] = out5[w];
        safe_permuted(calls, n_calls, walk);
    }
    if (states != nullptr) wave_store_records<5>(states, rec0, n, slab, st);
}

// ---- one sponge per WAVE (latency: a few sponges) -----------------------------------------------------------------------
// As k_sponge_lanes / k_cipher_lanes: lanes 0..4 hold the state (lane w = word w), lane 1 + p serves position p of a step.
// The helped form needs the same number of permutations from every wave of a block: n_perms for every sponge here.
template <bool HELPED>
__global__ void __launch_bounds__(kLanesWaves *kWave) k_safe_lanes(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                                   uint8_t *states, size_t n, size_t n_in, size_t n_out,
                                                                   SafeCalls calls, uint32_t n_calls, uint32_t cursor,
                                                                   uint32_t n_perms, Fr tag) {
    __shared__ LanesLds L[kLanesWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    constexpr int kPer = HELPED ? kLanesWaves - 1 : kLanesWaves;
    const size_t me = (size_t)blockIdx.x * kPer + wave;
    if constexpr (HELPED) {
        if (wave == kPer) {
            for (uint32_t t = 0; t < n_perms; t++) lanes_helper<kPer>(&d_lanes, *reinterpret_cast<LanesLds(*)[kPer]>(L));
            return;
        }
        if (me >= n) {
            for (uint32_t t = 0; t < n_perms; t++) lanes_idle();
            return;
        }
    } else {
        if (me >= n) return;
    }
    const uint8_t *src = in + me * n_in * 32;
    uint8_t *dst = out + me * n_out * 32;
    // (the one-shot call has no states, and an offset from a null pointer may not even be formed)
    uint8_t *mine = states != nullptr ? states + me * 160 + (lane < 5 ? lane : 0) * 32 : nullptr;
    const int p = lane - 1;                                            // the position this lane serves (0 .. 3: a word)
    Fr st = lane == 0 ? tag : zero_word();
    if (states != nullptr && lane < 5) st = load_word(mine);
    SafeWalk walk = safe_begin(calls, cursor);
    size_t in_off = 0, out_off = 0;
#pragma unroll 1
    for (uint32_t t = 0;; t++) {
        const SafeStep s = safe_step(calls, n_calls, walk);
        if (p >= s.e0 && p < s.e0 + s.j) store_word(dst + (out_off + (size_t)(p - s.e0)) * 32, st);
        if (p >= s.a0 && p < s.a0 + s.k) st = fr_add(st, load_word(src + (in_off + (size_t)(p - s.a0)) * 32));
        out_off += s.j;
        in_off += s.k;
        if (t == n_perms) break;
        st = lanes_perm<HELPED>(&d_lanes, L[wave], st);
        safe_permuted(calls, n_calls, walk);
    }
    if (states != nullptr && lane < 5) store_word(mine, st);
}
