// kernels_grind.hpp -- batched proof-of-work grinding over the permutation: the smallest nonce whose digest is below a target
// Part of the single translation unit hades252.hip (included there after kernels_safe.hpp); not a stand-alone header.
#pragma once

// Nothing in the reference tree defines a proof of work: the definition below is this repository's own, pinned only to its
// model (tests/grind_model.py): CONVENTION UNPINNED.  A job is a seed state of five words.  For a nonce x < 2^64
//   candidate(x) = seed with seed[word] + x (mod p) in place of seed[word]
//   digest(x)    = the canonical integer (what to_bytes gives, not the Montgomery limbs) of word out_idx of perm(candidate(x))
//   x is a hit  <=>  digest(x) < target     (strictly; target any 256-bit integer)
// and the answer is the SMALLEST hit of a nonce range.  In sponge terms: one absorb of x into a rate word of a resident
// state, one permutation, one word squeezed (kernels_sponge.hpp, kernels_safe.hpp), so the calls the library already has
// verify a nonce.
//
// The first kernel here with no memory traffic per candidate: the seed and the target are wave-uniform (scalar loads and
// kernel arguments), candidates are made in registers, ONE word leaves the round loop (fast_perm<1>) and nothing is staged
// through LDS.  What is left is fast_perm itself plus, per candidate, one Montgomery product (x -> x R), one addition, one
// to-bytes product and a compare: about 1 % of the permutation.
//
// Slots: one 64-bit word per job in device memory, all-ones = no hit yet, otherwise the smallest hit posted so far as an
// OFFSET from the call's first nonce (an offset is at most 2^64 - 2, so all-ones is never one).  A hit posts atomicMin (a
// vector global atomic; hits are rare).  Order independence: a wave gives up only when the slot is already below the
// smallest offset it has left, i.e. when nothing it could still post would change the minimum; a wave with an offset below
// the current best always evaluates it.  So the final slot is the minimum over ALL hits of the ranges launched so far,
// whatever the grid, the dispatch order or the moment at which any wave read the slot.

struct GrindTarget {
    uint32_t l[8];                            // canonical 256-bit integer, little-endian 32-bit limbs
};

// x R mod p for a 64-bit integer x: one Montgomery product with R^2
__device__ __forceinline__ Fr grind_nonce_mont(uint64_t x) {
    Fr a = zero_word(), r2;
    a.l[0] = (uint32_t)x;
    a.l[1] = (uint32_t)(x >> 32);
#pragma unroll
    for (int i = 0; i < 8; i++) r2.l[i] = d_r2[i];
    return fr_mul(a, r2);
}

// a < t as 256-bit integers, limb by limb from the top: the first limb that differs decides
__device__ __forceinline__ bool grind_below(const Fr &a, const GrindTarget &t) {
    bool below = false, decided = false;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        const bool differ = a.l[k] != t.l[k];
        below = (!decided && differ) ? a.l[k] < t.l[k] : below;
        decided = decided || differ;
    }
    return below;
}

// Grid: x = blocks of one job's window, y = the job.  Block b owns the offsets [b * iters * 256, (b + 1) * iters * 256) of
// the window [off0, off0 + count) and a lane walks them with stride 256, so earlier iterations hold smaller nonces.
// seeds: n_jobs x 160 B (Montgomery limbs); slots: n_jobs x 8 B.  nonce = first + offset never wraps: the host has checked
// first + max_nonces <= 2^64 and off0 + count <= max_nonces.
__global__ void __launch_bounds__(kBlock, 4) k_grind(const uint32_t *__restrict__ seeds, unsigned long long *slots,
                                                     GrindTarget target, int word, int out_idx, uint64_t first,
                                                     uint64_t off0, uint64_t count, uint32_t iters) {
    const uint32_t *seed = seeds + (size_t)blockIdx.y * 40;                  // uniform per block: scalar loads
    unsigned long long *slot = slots + blockIdx.y;
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x & ~(uint32_t)(kWave - 1));
    const uint32_t lane = threadIdx.x & (kWave - 1);
    uint64_t idx = (uint64_t)blockIdx.x * iters * kBlock + wave0;            // this wave's smallest index left in the window
#pragma unroll 1
    for (uint32_t it = 0; it < iters; it++, idx += kBlock) {
        if (idx >= count) return;
        // (relaxed, device scope: read again in every iteration, never hoisted)
        const unsigned long long best = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (best < off0 + idx) return;
        const uint64_t off = off0 + idx + lane;
        Fr st[5];
#pragma unroll
        for (int w = 0; w < 5; w++)
#pragma unroll
            for (int k = 0; k < 8; k++) st[w].l[k] = seed[w * 8 + k];
        Fr base = st[0];
#pragma unroll
        for (int w = 1; w < 5; w++)
            if (word == w) base = st[w];
        const Fr sum = fr_add(base, grind_nonce_mont(first + off));
#pragma unroll
        for (int w = 0; w < 5; w++)
            if (word == w) st[w] = sum;
        Fr out[1];
        fast_perm<1>(&d_fast, st, out, out_idx);
        const Fr digest = finalize1(mont_mul_small(to_f29(out[0]), kRpOverR));
        if (idx + lane < count && grind_below(digest, target)) atomicMin(slot, (unsigned long long)off);
    }
}
