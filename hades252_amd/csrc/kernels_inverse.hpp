// kernels_inverse.hpp -- the permutation run backwards, one state per lane, and batched fifth roots, one scalar per lane.
// Part of the single translation unit hades252.hip (included there after kernels_grind.hpp); not a stand-alone header.
#pragma once

// Round r of the reference (src/strategies.rs:79-157) is: add the round keys, x -> x^5 (every word in a full round, the last
// word in a partial one), multiply by the Cauchy matrix M.  Its inverse: multiply by M^-1, x -> x^D with D = 5^-1 mod (p - 1)
// on the same words, subtract the keys.  perm_inverse undoes rounds 66 .. 0.
//
// Arithmetic: the radix-2^29 Montgomery products of hades_fast.hpp.  Unlike the forward kernel nothing is scale-tracked:
// a word is held as value * Rp (Rp = 2^261, the radix of mont_fips), so mont_mul of two words is a word again, and M^-1 is
// dense -- 25 general constants, no small-integer form.  Constants are stored times Rp (hades252_amd/_derive.py::
// inverse_tables); one product on entry takes the in-memory word (value * 2^256) to value * Rp, one on exit takes it back.
//
// The fifth root is the whole cost: 99 of them per state (8 full rounds x 5 + 59 partial rounds).  The chain is a sliding
// window from the top bit of D over the table {x, x^3, x^5, x^7, x^51} (51 = 110011b: the low 100 bits of D repeat
// 0011 / 1100): 9 products for the table, 251 squarings, 51 multiplications -- HADES_INV_CHAIN_PRODUCTS = 311 products per
// root (plain square-and-multiply: 382).  The steps are DATA (d_inv.chain, wave-uniform scalar loads) walked by ONE loop
// whose body holds one squaring and one multiplication, and the table lives in registers: an entry is picked by comparing
// the step's index, never by indexing an array with it (that would put the table into scratch).  A state's five words go
// through the one copy of the chain by rotating the state (rotate_right, device_tables.hpp), as M^-1's five rows do.
//
// Bounds (hades_fast.hpp: mont_fips wants |limb| < 1.5 * 2^29 and |value| < 2^257; it returns normalised limbs and a value
// in (a b / Rp - p, a b / Rp]).  With a constant b < p and |a| < 2^257 a product lies in (-p - 2^251, 2^251).
//   after M^-1   the five products of a row are summed onto 2p with a carry pass after each: normalised, in
//                (-3p - 2^253.4, 2p + 2^253.4), below 1.6 * 2^256 in magnitude
//   after a root normalised, in (-p - 2^253, 2^253)
//   after a key  + (p - key) Rp mod p in balanced limbs: lazy limbs in [-2^28, 2^29 + 2^28), |value| < 3p + 2^253.4 < 2^257
//   on exit      x = word * 2^256 / Rp lies in (-p - 2^250.5, 2^250.5): finalize needs x + 2p in [0, 3p) and below 2^256

#ifndef HADES_INV_MINW
#define HADES_INV_MINW 3
#endif

struct InvTables {
    int32_t minv[5][5][kNL];              // M^-1[i][j] * Rp
    int32_t negkey[67][5][kNL];           // (p - key) * Rp, balanced limbs
    int32_t to_rp[kNL], from_rp[kNL];
    int32_t chain[HADES_INV_CHAIN_STEPS]; // 8 * squarings + table index
};
// (__constant__ and not const: every access is wave-uniform and arrives by scalar loads -- k_perm_fast.hpp, d_fast)
__constant__ InvTables d_inv = {HADES_INV_MINV_INIT, HADES_INV_NEGKEY_INIT, HADES_INV_TO_RP, HADES_INV_FROM_RP, HADES_INV_CHAIN_INIT};

__device__ __forceinline__ void inv_fence(F29 &x) {
#pragma unroll
    for (int k = 0; k < kNL; k++) limb_fence(x.l[k]);
}

// limbs 0..7 back into [0, 2^29), the top limb takes what is left (signed); the value is unchanged
__device__ __forceinline__ void inv_carry(F29 &x) {
#pragma unroll
    for (int k = 0; k < kNL - 1; k++) {
        const int32_t v = x.l[k];
        x.l[k] = (int32_t)((uint32_t)v & kMask29);
        x.l[k + 1] += v >> kLB;
    }
}

// entry k of the chain's table; k is wave-uniform
__device__ __forceinline__ F29 inv_pick(const F29 (&tab)[5], int k) {
    F29 m;
    // Limb by limb on FENCED values: left as a choice between loads of the table, hipcc turns it into one load at a chosen
    // address (the choice is made before the limb loop is unrolled), and the table then lives in scratch.
#pragma unroll
    for (int i = 0; i < kNL; i++) {
        int32_t e[5];
#pragma unroll
        for (int j = 0; j < 5; j++) {
            e[j] = tab[j].l[i];
            limb_fence(e[j]);
        }
        int32_t v = e[0];
        v = k == 1 ? e[1] : v;
        v = k == 2 ? e[2] : v;
        v = k == 3 ? e[3] : v;
        v = k == 4 ? e[4] : v;
        m.l[i] = v;
    }
    return m;
}

// x -> x^D (all values times Rp): HADES_INV_CHAIN_PRODUCTS products.  0 -> 0: every product of a multiple of p is one.
__device__ __forceinline__ F29 inv_fifth_root(const InvTables *T, const F29 &x) {
    F29 tab[5];
    tab[0] = x;
    const F29 x2 = mont_sqr(x);
    tab[1] = mont_mul(x2, x);
    tab[2] = mont_mul(tab[1], x2);
    tab[3] = mont_mul(tab[2], x2);
    F29 acc = tab[1];
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
        acc = mont_sqr(acc);
        inv_fence(acc);
    }
    tab[4] = mont_mul(acc, tab[1]);                              // x^51 = (x^3)^16 x^3
    acc = inv_pick(tab, T->chain[0] & 7);
#pragma unroll 1
    for (int s = 1; s < HADES_INV_CHAIN_STEPS; s++) {
        const int step = T->chain[s];
#pragma unroll 1
        for (int q = step >> 3; q > 0; q--) {
            acc = mont_sqr(acc);
            inv_fence(acc);
        }
        acc = mont_mul(acc, inv_pick(tab, step & 7));
        inv_fence(acc);
    }
    return acc;
}

// st <- M^-1 st, row by row through one code body: row i's sum enters at st'[4] while the rows before it move down
__device__ __forceinline__ void inv_linear(const InvTables *T, F29 (&st)[5]) {
    F29 out[5];
#pragma unroll
    for (int w = 0; w < 5; w++) out[w] = st[w];                  // (every entry is replaced below)
#pragma unroll 1
    for (int i = 0; i < 5; i++) {
        F29 sum;
#pragma unroll
        for (int k = 0; k < kNL; k++) sum.l[k] = TWOP29[k];
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const F29 t = mont_mul_const(st[j], T->minv[i][j]);
#pragma unroll
            for (int k = 0; k < kNL; k++) sum.l[k] += t.l[k];
            inv_carry(sum);
        }
        out[0] = out[1];
        out[1] = out[2];
        out[2] = out[3];
        out[3] = out[4];
        out[4] = sum;
#pragma unroll
        for (int w = 0; w < 5; w++) inv_fence(out[w]);
    }
#pragma unroll
    for (int w = 0; w < 5; w++) st[w] = out[w];
}

// The state after round round_hi - 1 (in-memory words) -> the state after round round_lo - 1, or the permutation's input for
// round_lo = 0.  0 <= round_lo <= round_hi <= 67, checked by the host.
__device__ __forceinline__ void inv_perm_rounds(const InvTables *T, Fr (&io)[5], int round_hi, int round_lo) {
    F29 st[5];
#pragma unroll
    for (int w = 0; w < 5; w++) st[w] = to_f29(io[w]);
#pragma unroll 1
    for (int w = 0; w < 5; w++) {
        st[4] = mont_mul_const(st[4], T->to_rp);
        rotate_right(st);
#pragma unroll
        for (int v = 0; v < 5; v++) inv_fence(st[v]);
    }
#pragma unroll 1
    for (int r = round_hi - 1; r >= round_lo; r--) {
        const bool full = r < 4 || r >= 63;
        inv_linear(T, st);
        const int roots = full ? 5 : 1;
#pragma unroll 1
        for (int i = 0; i < roots; i++) {
            st[4] = inv_fifth_root(T, st[4]);
            if (full) rotate_right(st);
#pragma unroll
            for (int v = 0; v < 5; v++) inv_fence(st[v]);
        }
#pragma unroll
        for (int w = 0; w < 5; w++) add_lazy(st[w], T->negkey[r][w]);
#pragma unroll
        for (int v = 0; v < 5; v++) inv_fence(st[v]);
    }
#pragma unroll 1
    for (int w = 0; w < 5; w++) {
        st[4] = mont_mul_const(st[4], T->from_rp);
        rotate_right(st);
#pragma unroll
        for (int v = 0; v < 5; v++) inv_fence(st[v]);
    }
#pragma unroll
    for (int w = 0; w < 5; w++) io[w] = finalize(st[w]);
}

// __launch_bounds__(256, 3): at least 3 waves per SIMD, i.e. at most 168 VGPRs; the 45 KB staging slab of a block admits 3
// blocks per CU as well.  In place: a wave has loaded all of its records before it stores any (staging.hpp).  Lanes past
// the end take part in the staging barriers and skip the arithmetic.
__global__ void __launch_bounds__(kBlock, HADES_INV_MINW) k_perm_inverse(uint8_t *states, size_t n, int round_hi, int round_lo) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *slab = wave_slab<5>(lds);
    const size_t rec0 = (size_t)blockIdx.x * kBlock + (threadIdx.x / kWave) * kWave;
    Fr st[5];
    wave_load_records<5>(states, rec0, n, slab, st);
    if (rec0 + (threadIdx.x & (kWave - 1)) < n) inv_perm_rounds(&d_inv, st, round_hi, round_lo);
    wave_store_records<5>(states, rec0, n, slab, st);
}

// One 32-byte scalar per lane, in place: consecutive lanes own consecutive scalars, so a wave's two 16-byte loads per lane
// cover 2 KiB contiguous.  No LDS.
__global__ void __launch_bounds__(kBlock, HADES_INV_MINW) k_fifth_root(uint8_t *scalars, size_t n) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    F29 x = mont_mul_const(to_f29(load_word(scalars + i * 32)), d_inv.to_rp);
    x = inv_fifth_root(&d_inv, x);
    store_word(scalars + i * 32, finalize(mont_mul_const(x, d_inv.from_rp)));
}
