// matrix_main.cpp -- the shipped kernel of hades252_amd/csrc/kernels_matrix.hpp as a host program, for the CPU-tier test
// tests/test_matrix_cpu_run.py (built with ASan + UBSan and run as an ordinary child process).
//
// <hip/hip_runtime.h> resolves to the stand-in of tests/hostsim (block emulator: see there); the tree's headers are the
// copies tests/hostsim_lib.py makes (rewritten(): the empty fences and the dynamic LDS declaration, nothing else).  Nothing
// in this file does arithmetic or defines a kernel or a device routine: it reads the planes, launches k_sponge_planes with
// the geometry of its call site in host_matrix.hpp and writes the digests.  The planes are a heap block of exactly
// ((N_COLS - 1) * STRIDE + N_ROWS) * 32 bytes -- the last plane ends with its last row -- and the gap between two planes
// (rows N_ROWS .. STRIDE - 1) is poisoned, so a read past ANY plane's last row is an ASan report; the digests are a heap
// block of exactly N_ROWS * 32 bytes.
//
//   matrix_main IN OUT N_ROWS N_COLS STRIDE PAD_MODE CAP0 CAP1 CAP2 CAP3       (the capacity's four limbs)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define MATRIX_POISON(p, n) __asan_poison_memory_region((p), (n))
#define MATRIX_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef MATRIX_POISON
#define MATRIX_POISON(p, n) ((void)0)
#define MATRIX_UNPOISON(p, n) ((void)0)
#endif

#include "include/hades252.h"
#include "hades252_amd/csrc/fr32.hpp"
#include "hades252_amd/csrc/hades_constants.inc"
#include "hades252_amd/csrc/hades_literal.hpp"
#include "hades252_amd/csrc/staging.hpp"
#include "hades252_amd/csrc/hades_fast.hpp"
#include "hades252_amd/csrc/k_perm_fast.hpp"
#include "hades252_amd/csrc/hades_coop.hpp"
#include "hades252_amd/csrc/hades_lanes.hpp"

using namespace hades;

#include "hades252_amd/csrc/device_tables.hpp"
#include "hades252_amd/csrc/kernels_matrix.hpp"

static int usage() {
    fprintf(stderr, "usage: matrix_main IN OUT N_ROWS N_COLS STRIDE PAD_MODE CAP0 CAP1 CAP2 CAP3\n");
    return 2;
}

int main(int argc, char **argv) {
    if (argc != 11) return usage();
    const size_t n_rows = (size_t)strtoull(argv[3], nullptr, 0), n_cols = (size_t)strtoull(argv[4], nullptr, 0);
    const size_t stride = (size_t)strtoull(argv[5], nullptr, 0);
    const int pad_mode = atoi(argv[6]);
    if (n_rows == 0 || n_cols == 0 || stride < n_rows || (pad_mode != 0 && pad_mode != 1)) return usage();
    Fr cap;
    for (int k = 0; k < 4; k++) {
        const uint64_t v = strtoull(argv[7 + k], nullptr, 0);
        cap.l[2 * k] = (uint32_t)v;
        cap.l[2 * k + 1] = (uint32_t)(v >> 32);
    }
    const size_t bytes = ((n_cols - 1) * stride + n_rows) * 32, out_bytes = n_rows * 32;
    FILE *f = fopen(argv[1], "rb");
    if (f == nullptr) return usage();
    uint8_t *planes = nullptr, *digests = nullptr;
    if (posix_memalign((void **)&planes, 16, bytes) != 0 || posix_memalign((void **)&digests, 16, out_bytes) != 0) return 3;
    const size_t got = fread(planes, 1, bytes, f);
    const bool more = fgetc(f) != EOF;
    fclose(f);
    if (got != bytes || more) {
        fprintf(stderr, "matrix_main: %s does not hold exactly %zu bytes\n", argv[1], bytes);
        return 3;
    }
    memset(digests, 0xA5, out_bytes);
    for (size_t c = 0; c + 1 < n_cols; c++) MATRIX_POISON(planes + (c * stride + n_rows) * 32, (stride - n_rows) * 32);
    const size_t m = n_rows;
    hipLaunchKernelGGL(k_sponge_planes, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t) nullptr, planes,
                       m, n_cols, stride, digests, cap, pad_mode);
    for (size_t c = 0; c + 1 < n_cols; c++) MATRIX_UNPOISON(planes + (c * stride + n_rows) * 32, (stride - n_rows) * 32);
    f = fopen(argv[2], "wb");
    if (f == nullptr || fwrite(digests, 1, out_bytes, f) != out_bytes) return 4;
    fclose(f);
    free(planes);
    free(digests);
    free(hostsim::g_lds_arena);
    hostsim::g_lds_arena = nullptr;
    return 0;
}
