// kernels_cipher.hpp -- batched Poseidon cipher (authenticated encryption over the permutation): one message per lane, one per wave
// Part of the single translation unit hades252.hip (included there after kernels_sponge.hpp); not a stand-alone header.
#pragma once

// The third caller of `perm` in dusk-poseidon (reference README.md:9): PoseidonCipher, which Dusk uses for note payloads.
// That crate is NOT part of the reference tree; the construction below is recalled from it (<= 0.33), the domain word is a
// call parameter and parity is pinned only to this repository's model (tests/cipher_model.py): CONVENTION UNPINNED.
//   state = [D, M, kx, ky, nonce]        (M = the field element M, Montgomery form like every other word)
//   encrypt: for every block b of four words: perm; words 1..4 += m[4b .. 4b+4) (the words that exist); c[4b + j] = word 1 + j
//            then perm; c[M] = word 1 (the tag): M + 1 words out
//   decrypt: the same chain, m[4b + j] = c[4b + j] - word 1 + j, word 1 + j = c[4b + j]; then perm; ok = (c[M] == word 1)
//            and every c word canonical (< p as a 256-bit integer); a rejected message comes out as M zero words.
// The crate's instance is M = 2, D = 2^32; for M <= 4 ceil(M / 4) agrees with its block count, for larger M this is the
// natural generalisation (one permutation per block of four words).
// Encrypt inputs must be canonical (a precondition, as for perm); decrypt checks its cipher words, which come from outside.

// a - b mod p (a, b fully reduced): borrow chain, then + p where it borrowed
__device__ __forceinline__ Fr fr_sub(const Fr &a, const Fr &b) {
    Fr d, s;
    unsigned borrow = 0, carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        unsigned bo;
        d.l[i] = __builtin_subc(a.l[i], b.l[i], borrow, &bo);
        borrow = bo;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        unsigned co;
        s.l[i] = __builtin_addc(d.l[i], FR_P[i], carry, &co);
        carry = co;
    }
    return fr_select(borrow != 0, s, d);
}

// a == b as 256-bit integers
__device__ __forceinline__ bool fr_eq(const Fr &a, const Fr &b) {
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) x |= a.l[i] ^ b.l[i];
    return x == 0;
}

// ---- one message per lane (throughput) ---------------------------------------------------------------------------
// Every message of a launch has the same length, so the block loop is uniform across the wave.  Message / cipher words
// are AoS with `stride` words per message; words [first, first + cnt) (cnt <= 4, the same for every message) of the
// wave's 64 messages move through the wave's LDS slab: 8 lanes carry the (up to) 128 contiguous bytes of one message,
// 8 messages per instruction -- no lane walks HBM with a message-sized stride.  The slab is wave-private and a wave's LDS
// operations execute in order: compiler fences only (as in k_sponge).
// `lo` (0 for the cipher) shifts the slots: the words land in w[lo .. lo + cnt), the other slots read zero (the duplex
// sponge of kernels_safe.hpp resumes a block at position lo).
__device__ __forceinline__ void cipher_gather(const uint8_t *base, size_t stride, size_t first, int cnt, size_t rec0, size_t n,
                                              uint8_t *slab, Fr (&w)[4], int lo = 0) {
    constexpr int kRec = lds_rec_bytes(4);
    const int lane = threadIdx.x & (kWave - 1), part = lane & 7, j = part >> 1;
    // message 8k + lane / 8: one per-lane offset, a wave-uniform step of 8 messages.  (An offset, not a pointer: for a slot
    // j < lo it wraps to before the message -- never read -- and C++ does not allow such a pointer even to be formed.)
    const size_t off = ((rec0 + (lane >> 3)) * stride + first + j - lo) * 32 + (part & 1) * 16;
    const size_t step = 8 * stride * 32;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int m = 8 * k + (lane >> 3);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (j >= lo && j < lo + cnt && rec0 + m < n) v = *reinterpret_cast<const uint4 *>(base + off + k * step);
        *reinterpret_cast<uint4 *>(slab + m * kRec + part * 16) = v;
    }
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 *p = reinterpret_cast<const uint4 *>(slab + lane * kRec + k * 32);
        const uint4 lo = p[0], hi = p[1];
        w[k].l[0] = lo.x; w[k].l[1] = lo.y; w[k].l[2] = lo.z; w[k].l[3] = lo.w;
        w[k].l[4] = hi.x; w[k].l[5] = hi.y; w[k].l[6] = hi.z; w[k].l[7] = hi.w;
    }
    wave_lds_fence();
}

// The reverse: w[lo .. lo + cnt) of every lane -> words [first, first + cnt) of its message.  With ZERO_BAD, zeros go to the
// messages whose owner lane has bad set, nothing to the others (the lane that stores a given address is the same in
// both forms, so a zeroing pass is ordered after the earlier store by program order).
template <bool ZERO_BAD>
__device__ __forceinline__ void cipher_scatter(uint8_t *base, size_t stride, size_t first, int cnt, size_t rec0, size_t n,
                                               uint8_t *slab, const Fr (&w)[4], bool bad = false, int lo = 0) {
    constexpr int kRec = lds_rec_bytes(4);
    const int lane = threadIdx.x & (kWave - 1), part = lane & 7, j = part >> 1;
    if constexpr (!ZERO_BAD) {
#pragma unroll
        for (int k = 0; k < 4; k++) slab_put<4>(slab, k, w[k]);
        wave_lds_fence();
    }
    const uint64_t bad_mask = ZERO_BAD ? __ballot(bad) : 0;
    const size_t off = ((rec0 + (lane >> 3)) * stride + first + j - lo) * 32 + (part & 1) * 16;   // (see cipher_gather)
    const size_t step = 8 * stride * 32;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int m = 8 * k + (lane >> 3);
        uint4 v = make_uint4(0, 0, 0, 0);
        if constexpr (!ZERO_BAD) v = *reinterpret_cast<const uint4 *>(slab + m * kRec + part * 16);
        const bool go = ZERO_BAD ? ((bad_mask >> m) & 1) != 0 : true;
        if (go && j >= lo && j < lo + cnt && rec0 + m < n) *reinterpret_cast<uint4 *>(base + off + k * step) = v;
    }
    if constexpr (!ZERO_BAD) wave_lds_fence();
}

// DECRYPT = false: in = messages (len words each), out = ciphers (len + 1).  DECRYPT = true: in = ciphers, out = messages,
// ok_out[i] = 1 / 0, *rejected += rejections (may be NULL).  Decrypt is branch-free on ok: every message's words are
// stored block by block, and after the tag check a zeroing pass, whose instructions every wave runs whatever its
// messages' verdicts, overwrites the words of the rejected ones (only their stores are enabled).  Holding the message
// in registers until the verdict instead would keep 32 more VGPRs live across the permutation (spills).
template <bool DECRYPT>
__global__ void __launch_bounds__(kBlock, 3) k_cipher(const uint8_t *__restrict__ in, const uint8_t *__restrict__ keys,
                                                      const uint8_t *__restrict__ nonces, uint8_t *__restrict__ out,
                                                      uint8_t *__restrict__ ok_out, int *rejected, size_t n, size_t len,
                                                      Fr domain, Fr len_word) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *slab = wave_slab<4>(lds);
    const int lane = threadIdx.x & (kWave - 1);
    const size_t rec0 = (size_t)blockIdx.x * kBlock + (threadIdx.x / kWave) * kWave;
    const bool live = rec0 + lane < n;
    Fr key[2], nonce[1];
    wave_load_records<2>(keys, rec0, n, slab, key);          // (block-wide barriers: every wave of the block gets here)
    wave_load_records<1>(nonces, rec0, n, slab, nonce);
    Fr st[5] = {domain, len_word, key[0], key[1], nonce[0]};
    const size_t in_stride = DECRYPT ? len + 1 : len, out_stride = DECRYPT ? len : len + 1;
    const uint64_t blocks = (len + 3) / 4;
    bool good = true;
    // blocks + 1 permutations through ONE call site (the loop body stays inside the instruction cache, as in k_sponge)
#pragma unroll 1
    for (uint64_t b = 0;; b++) {
        Fr out5[5];
        fast_perm<5>(&d_fast, st, out5, 0);
#pragma unroll
        for (int w = 0; w < 5; w++) st[w] = out5[w];
        if (b == blocks) break;
        const int cnt = len - 4 * b < 4 ? (int)(len - 4 * b) : 4;
        Fr w4[4], o4[4];
        cipher_gather(in, in_stride, 4 * b, cnt, rec0, n, slab, w4);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            o4[j] = zero_word();
            if (j < cnt) {
                if constexpr (DECRYPT) {
                    good = good && fr_is_canonical(w4[j]);
                    o4[j] = fr_sub(w4[j], st[1 + j]);
                    st[1 + j] = w4[j];
                } else {
                    st[1 + j] = fr_add(st[1 + j], w4[j]);
                    o4[j] = st[1 + j];
                }
            }
        }
        cipher_scatter<false>(out, out_stride, 4 * b, cnt, rec0, n, slab, o4);
    }
    Fr tag[4] = {st[1], st[1], st[1], st[1]};
    if constexpr (!DECRYPT) {
        cipher_scatter<false>(out, out_stride, len, 1, rec0, n, slab, tag);
    } else {
        Fr c4[4];
        cipher_gather(in, in_stride, len, 1, rec0, n, slab, c4);
        good = good && fr_is_canonical(c4[0]) && fr_eq(c4[0], tag[0]);
        // the zeroing pass: the same instructions for every wave, stores enabled for the rejected messages only
#pragma unroll 1
        for (uint64_t b = 0; b < blocks; b++) {
            const int cnt = len - 4 * b < 4 ? (int)(len - 4 * b) : 4;
            cipher_scatter<true>(out, out_stride, 4 * b, cnt, rec0, n, slab, tag, !good);
        }
        if (live) ok_out[rec0 + lane] = good ? 1 : 0;
        const uint64_t rej = __ballot(live && !good);
        if (lane == 0 && rej != 0 && rejected != nullptr) atomicAdd(rejected, (int)__popcll(rej));
    }
}

// ---- one message per WAVE (latency: a few messages) -----------------------------------------------------------------
// The cipher is a chain of dependent permutations per message: as k_sponge_lanes, lanes 0..4 hold the state (lane w =
// word w) and lane 1 + j the message / cipher word 4b + j of block b, fetched before the block's permutation.  The helped
// form needs the same number of permutations from every wave of a block: blocks + 1 for every message here.
template <bool DECRYPT, bool HELPED>
__global__ void __launch_bounds__(kLanesWaves *kWave) k_cipher_lanes(const uint8_t *__restrict__ in, const uint8_t *__restrict__ keys,
                                                                     const uint8_t *__restrict__ nonces, uint8_t *__restrict__ out,
                                                                     uint8_t *__restrict__ ok_out, int *rejected, size_t n,
                                                                     size_t len, Fr domain, Fr len_word) {
    __shared__ LanesLds L[kLanesWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    constexpr int kPer = HELPED ? kLanesWaves - 1 : kLanesWaves;
    const size_t me = (size_t)blockIdx.x * kPer + wave;
    const uint64_t blocks = (len + 3) / 4;
    if constexpr (HELPED) {
        if (wave == kPer) {
            for (uint64_t t = 0; t < blocks + 1; t++)
                lanes_helper<kPer>(&d_lanes, *reinterpret_cast<LanesLds(*)[kPer]>(L));
            return;
        }
        if (me >= n) {
            for (uint64_t t = 0; t < blocks + 1; t++) lanes_idle();
            return;
        }
    } else {
        if (me >= n) return;
    }
    const size_t in_stride = DECRYPT ? len + 1 : len, out_stride = DECRYPT ? len : len + 1;
    const uint8_t *src = in + me * in_stride * 32;
    uint8_t *dst = out + me * out_stride * 32;
    const bool word = lane >= 1 && lane <= 4;
    const uint64_t j = word ? (uint64_t)(lane - 1) : 0;
    Fr st = lane == 0 ? domain : lane == 1 ? len_word : zero_word();
    if (lane == 2 || lane == 3) st = load_word(keys + (me * 2 + (lane - 2)) * 32);
    if (lane == 4) st = load_word(nonces + me * 32);
    bool good = true;
#pragma unroll 1
    for (uint64_t b = 0; b < blocks; b++) {
        const uint64_t idx = 4 * b + j;
        const bool mine = word && idx < len;
        const Fr w = mine ? load_word(src + idx * 32) : zero_word();      // in flight during the permutation
        st = lanes_perm<HELPED>(&d_lanes, L[wave], st);
        if (mine) {
            if constexpr (DECRYPT) {
                good = good && fr_is_canonical(w);
                store_word(dst + idx * 32, fr_sub(w, st));
                st = w;
            } else {
                st = fr_add(st, w);
                store_word(dst + idx * 32, st);
            }
        }
    }
    const Fr tag = DECRYPT && lane == 1 ? load_word(src + len * 32) : zero_word();
    st = lanes_perm<HELPED>(&d_lanes, L[wave], st);
    if constexpr (!DECRYPT) {
        if (lane == 1) store_word(dst + len * 32, st);
    } else {
        if (lane == 1) good = good && fr_is_canonical(tag) && fr_eq(tag, st);
        const bool ok = __ballot(!good) == 0;                               // wave-uniform: one message per wave
        if (!ok) {                                                          // each word zeroed by the lane that stored it
#pragma unroll 1
            for (uint64_t b = 0; b < blocks; b++)
                if (word && 4 * b + j < len) store_word(dst + (4 * b + j) * 32, zero_word());
        }
        if (lane == 0) {
            ok_out[me] = ok ? 1 : 0;
            if (!ok && rejected != nullptr) atomicAdd(rejected, 1);
        }
    }
}
