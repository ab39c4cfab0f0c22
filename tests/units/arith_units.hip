// arith_units.hip -- test-only library: the device field routines of the shipped headers, one kernel each, so that
// tests/test_gpu_a13_units.py can drive them with chosen operands and compare them limb for limb with their Python
// models (tests/test_fast_model.py).  Built by tests/units_lib.py with the product's own hipcc flags.
//
// The headers are included unchanged, in the order of hades252_amd/csrc/hades252.hip.  Nothing here does arithmetic of
// its own: each kernel loads its operands, calls ONE shipped routine and stores what it returns.  (tests/test_units_lib.py
// checks that no wrapped routine is defined in this file.)
//
// Formats: F29 = 9 x int32 (signed limbs, lazy allowed), Fr = 8 x u32, a lane row = 16 x u32 (limb k in lane k).
// One element per lane; the lane routines take one element per 16-lane row (four per wave).  Every kernel checks its
// index against n before it reads or writes, and writes only its own element of its output.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/hades252.h"
#include "../../hades252_amd/csrc/fr32.hpp"
#include "../../hades252_amd/csrc/hades_constants.inc"
#include "../../hades252_amd/csrc/hades_literal.hpp"
#include "../../hades252_amd/csrc/staging.hpp"
#include "../../hades252_amd/csrc/hades_fast.hpp"
#include "../../hades252_amd/csrc/k_perm_fast.hpp"
#include "../../hades252_amd/csrc/hades_coop.hpp"
#include "../../hades252_amd/csrc/hades_lanes.hpp"

using namespace hades;

#include "../../hades252_amd/csrc/device_tables.hpp"
#include "../../hades252_amd/csrc/kernels_perm.hpp"

namespace {

constexpr int kUnitBlock = 256;

__device__ __forceinline__ size_t elem() { return (size_t)blockIdx.x * kUnitBlock + threadIdx.x; }

__device__ __forceinline__ F29 ld29(const int32_t *p, size_t i) {
    F29 r;
#pragma unroll
    for (int k = 0; k < kNL; k++) r.l[k] = p[kNL * i + k];
    return r;
}
__device__ __forceinline__ void st29(int32_t *p, size_t i, const F29 &v) {
#pragma unroll
    for (int k = 0; k < kNL; k++) p[kNL * i + k] = v.l[k];
}
__device__ __forceinline__ Fr ld32(const uint32_t *p, size_t i) {
    Fr r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = p[8 * i + k];
    return r;
}
__device__ __forceinline__ void st32(uint32_t *p, size_t i, const Fr &v) {
#pragma unroll
    for (int k = 0; k < 8; k++) p[8 * i + k] = v.l[k];
}
__device__ __forceinline__ LaneConsts lane_consts() {
    LaneConsts K;
#pragma unroll
    for (int i = 0; i < kNL; i++) {
        K.p[i] = d_lanes.p[i];
        K.pinv[i] = d_lanes.pinv[i];
    }
    return K;
}

// ---- hades_fast.hpp ----------------------------------------------------------------------------------------------
__global__ void u_to_f29(const uint32_t *a, int32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st29(out, i, to_f29(ld32(a, i)));
}
__global__ void u_from_f29(const int32_t *a, uint32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st32(out, i, from_f29(ld29(a, i)));
}
__global__ void u_mont_mul(const int32_t *a, const int32_t *b, int32_t *out, size_t n) {
    const size_t i = elem();
    if (i >= n) return;
    const F29 x = ld29(a, i), y = ld29(b, i);
    st29(out, i, mont_fips<false, false>(x, y.l));
}
__global__ void u_mont_sqr(const int32_t *a, int32_t *out, size_t n) {
    const size_t i = elem();
    if (i >= n) return;
    const F29 x = ld29(a, i);
    st29(out, i, mont_fips<true, false>(x, x.l));
}
__global__ void u_mont_mul_const(const int32_t *a, const int32_t *c, int32_t *out, size_t n) {   // c: 9 limbs, uniform
    const size_t i = elem();
    if (i < n) st29(out, i, mont_fips<false, true>(ld29(a, i), c));
}
__global__ void u_mont_mul_small(const int32_t *a, const int32_t *c, int32_t *out, size_t n) {   // c: one per element
    const size_t i = elem();
    if (i < n) st29(out, i, mont_mul_small(ld29(a, i), c[i]));
}
__global__ void u_mont_lin(const int32_t *a, const int32_t *e, int32_t *out, size_t n) {   // e: 81-entry table, uniform
    const size_t i = elem();
    if (i < n) st29(out, i, mont_lin(ld29(a, i), e));
}
__global__ void u_mont_lin1(const int32_t *a, const int32_t *e, int32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st29(out, i, mont_lin1(ld29(a, i), e));
}
__global__ void u_sbox29(const int32_t *a, int32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st29(out, i, sbox29(ld29(a, i)));
}
__global__ void u_add_lazy(const int32_t *a, const int32_t *c, int32_t *out, size_t n) {
    const size_t i = elem();
    if (i >= n) return;
    F29 x = ld29(a, i);
    const F29 y = ld29(c, i);
    add_lazy(x, y.l);
    st29(out, i, x);
}
__global__ void u_small_mds(const int32_t *st, int32_t *out, size_t n) {   // five words per element
    const size_t i = elem();
    if (i >= n) return;
    F29 s[5];
#pragma unroll
    for (int w = 0; w < 5; w++) s[w] = ld29(st, 5 * i + w);
    small_mds(s);
#pragma unroll
    for (int w = 0; w < 5; w++) st29(out, 5 * i + w, s[w]);
}
__global__ void u_finalize(const int32_t *a, uint32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st32(out, i, finalize(ld29(a, i)));
}
__global__ void u_finalize1(const int32_t *a, uint32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st32(out, i, finalize1(ld29(a, i)));
}

// ---- kernels_perm.hpp --------------------------------------------------------------------------------------------
__global__ void u_finalize32(const int32_t *a, uint32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st32(out, i, finalize32(ld29(a, i)));
}
template <int NCOL>
__global__ void u_mds_row_cols(const int32_t *u, int row, int32_t *out, size_t n) {   // row: wave-uniform, as in the kernel
    const size_t i = elem();
    if (i >= n) return;
    F29 s[5];
#pragma unroll
    for (int w = 0; w < 5; w++) s[w] = ld29(u, 5 * i + w);
    st29(out, i, mds_row_cols<NCOL>(d_coop.mds[row], s));
}

// ---- fr32.hpp ----------------------------------------------------------------------------------------------------
__global__ void u_fr_add(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st32(out, i, fr_add(ld32(a, i), ld32(b, i)));
}
__global__ void u_fr_cond_sub_p(const uint32_t *a, const uint32_t *top, uint32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st32(out, i, fr_cond_sub_p(ld32(a, i), top[i]));
}
__global__ void u_fr_mul(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) st32(out, i, fr_mul(ld32(a, i), ld32(b, i)));
}
__global__ void u_fr_is_canonical(const uint32_t *a, uint32_t *out, size_t n) {
    const size_t i = elem();
    if (i < n) out[i] = fr_is_canonical(ld32(a, i)) ? 1u : 0u;
}

// ---- hades_lanes.hpp: one element per 16-lane row; a row is wholly in or wholly out of range ---------------------
__device__ __forceinline__ bool row_of(size_t n, size_t &row, int &lane) {
    const size_t t = elem();
    row = t >> 4;
    lane = (int)(threadIdx.x & 15);
    return row < n;
}
__global__ void u_lane_mont_mul(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n) {
    size_t r;
    int k;
    if (!row_of(n, r, k)) return;
    out[16 * r + k] = lane_mont_mul(lane_consts(), a[16 * r + k], b[16 * r + k]);
}
__global__ void u_lane_sbox(const uint32_t *a, uint32_t *out, size_t n) {
    size_t r;
    int k;
    if (!row_of(n, r, k)) return;
    out[16 * r + k] = lane_sbox(lane_consts(), a[16 * r + k]);
}
// e: [9][16] per-lane table (lane j of e[k] = limb j of E_k), as the rows kernel reads d_rows_klin
__global__ void u_lane_lin(const uint32_t *a, const uint32_t *e, uint32_t *out, size_t n) {
    size_t r;
    int k;
    if (!row_of(n, r, k)) return;
    uint32_t ek[kNL];
#pragma unroll
    for (int j = 0; j < kNL; j++) ek[j] = e[16 * j + k];
    const uint32_t pk = d_lanes.p16[k], pk1 = row_shr<1>(pk);
    out[16 * r + k] = lane_lin(lane_consts(), a[16 * r + k], ek, pk, pk1);
}
__global__ void u_lane_mds_row(const uint32_t *x, int row, uint32_t *out, size_t n) {   // five rows per element
    size_t r;
    int k;
    if (!row_of(n, r, k)) return;
    uint32_t c[5], xs[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        c[j] = d_lanes.mds[row][j];
        xs[j] = x[16 * (5 * r + j) + k];
    }
    out[16 * r + k] = lane_mds_row(c, xs, d_lanes.p16[k]);
}
__global__ void u_carry_split(const uint64_t *acc, uint32_t *t, uint32_t *c16, uint32_t *c17, size_t n) {
    size_t r;
    int k;
    if (!row_of(n, r, k)) return;
    uint32_t a, b;
    t[16 * r + k] = carry_split(acc[16 * r + k], a, b);
    c16[16 * r + k] = a;
    c17[16 * r + k] = b;
}

// ---- hades_lanes.hpp: the data moves themselves, one element per WAVE (64 lanes in, kDppMoves x 64 lanes out) --------
// results, 64 words each: row_shr<1..15>, row_shl<1..15>, row_bcast<0..15>, wave_bcast_row<0>, <1>, then both halves of
// v_permlane16_swap a, b and of v_permlane32_swap a, b (the raw builtins wave_bcast_row is made of, with d != s)
constexpr int kDppMoves = 52;
template <int N>
__device__ __forceinline__ void row_moves(uint32_t v, uint32_t *o) {
    if constexpr (N < 16) {
        if constexpr (N > 0) {
            o[64 * (N - 1)] = row_shr<N>(v);
            o[64 * (14 + N)] = row_shl<N>(v);
        }
        o[64 * (30 + N)] = row_bcast<N>(v);
        row_moves<N + 1>(v, o);
    }
}
__global__ void u_dpp_moves(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n) {
    const size_t t = elem(), w = t >> 6;                             // a wave is wholly in or wholly out of range
    if (w >= n) return;
    const uint32_t va = a[t], vb = b[t];
    uint32_t *o = out + w * (64 * kDppMoves) + (threadIdx.x & 63);
    row_moves<0>(va, o);
    o[64 * 46] = wave_bcast_row<0>(va);
    o[64 * 47] = wave_bcast_row<1>(va);
    const auto h = __builtin_amdgcn_permlane16_swap(va, vb, false, false);
    o[64 * 48] = h[0];
    o[64 * 49] = h[1];
    const auto q = __builtin_amdgcn_permlane32_swap(va, vb, false, false);
    o[64 * 50] = q[0];
    o[64 * 51] = q[1];
}

dim3 grid_for(size_t threads) { return dim3((unsigned)((threads + kUnitBlock - 1) / kUnitBlock)); }

int status() { return hipGetLastError() == hipSuccess ? 0 : -1; }

bool bad_n(size_t n) { return n == 0 || n > ((size_t)1 << 24); }

}  // namespace

// ---- launchers: device pointers, a count, a stream; 0 = launched, -1 = launch error, -2 = bad argument -------------
#define UNITS_LAUNCH(kernel, threads, ...)                                                                          \
    do {                                                                                                          \
        if (bad_n(n)) return -2;                                                                                  \
        hipLaunchKernelGGL(kernel, grid_for(threads), dim3(kUnitBlock), 0, (hipStream_t)stream, __VA_ARGS__);    \
        return status();                                                                                          \
    } while (0)

extern "C" {

int units_to_f29(const void *a, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_to_f29, n, (const uint32_t *)a, (int32_t *)out, n);
}
int units_from_f29(const void *a, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_from_f29, n, (const int32_t *)a, (uint32_t *)out, n);
}
int units_mont_mul(const void *a, const void *b, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_mont_mul, n, (const int32_t *)a, (const int32_t *)b, (int32_t *)out, n);
}
int units_mont_sqr(const void *a, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_mont_sqr, n, (const int32_t *)a, (int32_t *)out, n);
}
int units_mont_mul_const(const void *a, const void *c, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_mont_mul_const, n, (const int32_t *)a, (const int32_t *)c, (int32_t *)out, n);
}
int units_mont_mul_small(const void *a, const void *c, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_mont_mul_small, n, (const int32_t *)a, (const int32_t *)c, (int32_t *)out, n);
}
int units_mont_lin(const void *a, const void *e, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_mont_lin, n, (const int32_t *)a, (const int32_t *)e, (int32_t *)out, n);
}
int units_mont_lin1(const void *a, const void *e, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_mont_lin1, n, (const int32_t *)a, (const int32_t *)e, (int32_t *)out, n);
}
int units_sbox29(const void *a, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_sbox29, n, (const int32_t *)a, (int32_t *)out, n);
}
int units_add_lazy(const void *a, const void *c, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_add_lazy, n, (const int32_t *)a, (const int32_t *)c, (int32_t *)out, n);
}
int units_small_mds(const void *st, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_small_mds, n, (const int32_t *)st, (int32_t *)out, n);
}
int units_finalize(const void *a, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_finalize, n, (const int32_t *)a, (uint32_t *)out, n);
}
int units_finalize1(const void *a, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_finalize1, n, (const int32_t *)a, (uint32_t *)out, n);
}
int units_finalize32(const void *a, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_finalize32, n, (const int32_t *)a, (uint32_t *)out, n);
}
int units_mds_row_cols(int ncol, const void *u, int row, void *out, size_t n, void *stream) {
    if (row < 0 || row >= 5) return -2;
    if (ncol == 3) UNITS_LAUNCH(u_mds_row_cols<3>, n, (const int32_t *)u, row, (int32_t *)out, n);
    if (ncol == 5) UNITS_LAUNCH(u_mds_row_cols<5>, n, (const int32_t *)u, row, (int32_t *)out, n);
    return -2;
}
int units_fr_add(const void *a, const void *b, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_fr_add, n, (const uint32_t *)a, (const uint32_t *)b, (uint32_t *)out, n);
}
int units_fr_cond_sub_p(const void *a, const void *top, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_fr_cond_sub_p, n, (const uint32_t *)a, (const uint32_t *)top, (uint32_t *)out, n);
}
int units_fr_mul(const void *a, const void *b, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_fr_mul, n, (const uint32_t *)a, (const uint32_t *)b, (uint32_t *)out, n);
}
int units_fr_is_canonical(const void *a, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_fr_is_canonical, n, (const uint32_t *)a, (uint32_t *)out, n);
}
int units_lane_mont_mul(const void *a, const void *b, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_lane_mont_mul, 16 * n, (const uint32_t *)a, (const uint32_t *)b, (uint32_t *)out, n);
}
int units_lane_sbox(const void *a, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_lane_sbox, 16 * n, (const uint32_t *)a, (uint32_t *)out, n);
}
int units_lane_lin(const void *a, const void *e, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_lane_lin, 16 * n, (const uint32_t *)a, (const uint32_t *)e, (uint32_t *)out, n);
}
int units_lane_mds_row(const void *x, int row, void *out, size_t n, void *stream) {
    if (row < 0 || row >= 5) return -2;
    UNITS_LAUNCH(u_lane_mds_row, 16 * n, (const uint32_t *)x, row, (uint32_t *)out, n);
}
int units_carry_split(const void *acc, void *t, void *c16, void *c17, size_t n, void *stream) {
    UNITS_LAUNCH(u_carry_split, 16 * n, (const uint64_t *)acc, (uint32_t *)t, (uint32_t *)c16, (uint32_t *)c17, n);
}
int units_dpp_moves(const void *a, const void *b, void *out, size_t n, void *stream) {
    UNITS_LAUNCH(u_dpp_moves, 64 * n, (const uint32_t *)a, (const uint32_t *)b, (uint32_t *)out, n);
}

}  // extern "C"
