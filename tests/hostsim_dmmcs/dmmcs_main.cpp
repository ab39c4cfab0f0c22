// dmmcs_main.cpp -- the shipped kernels of hades252_amd/csrc/kernels_dmmcs.hpp as a host program, for the CPU-tier test
// tests/test_dmmcs_cpu_run.py (built with ASan + UBSan and run as an ordinary child process).
//
// <hip/hip_runtime.h> resolves to the stand-in of tests/hostsim (block emulator: see there); the tree's headers are the
// copies tests/hostsim_lib.py makes (rewritten(): the empty fences and the dynamic LDS declaration, nothing else).  Nothing
// in this file does arithmetic or defines a kernel or a device routine: it reads its inputs, fills the part table the way
// abi_dmmcs.hpp does (the blocks of all parts laid end to end, in the order given), launches k_dmmcs_absorb or k_dmmcs_rows
// with the geometry of its call site there and writes what the kernel wrote.  Every buffer is a heap block of exactly its
// size: the five state planes of a part (N_ROWS * 160 bytes), the indices (N * 8) and the output rows (N * ROW_COLS * 32);
// the planes of a part are a block of exactly ((G - 1) * STRIDE + N_ROWS) * 32 bytes -- the last plane ends with its last
// row -- and the gap between two planes (rows N_ROWS .. STRIDE - 1) is poisoned, so an access past ANY plane's last row, any
// state plane, the last index or the last output scalar is an ASan report.
//
//   dmmcs_main absorb OUT N_PARTS [STATE PLANES N_ROWS G STRIDE CUR]...     writes OUT.state.<p>: part p's state planes after
//   dmmcs_main rows OUT N H0 INDICES N_PARTS [PLANES N_ROWS COLS STRIDE]... writes OUT: N x (sum of COLS) scalars
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define DMMCS_POISON(p, n) __asan_poison_memory_region((p), (n))
#define DMMCS_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef DMMCS_POISON
#define DMMCS_POISON(p, n) ((void)0)
#define DMMCS_UNPOISON(p, n) ((void)0)
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
#include "hades252_amd/csrc/kernels_dmmcs.hpp"

static int usage() {
    fprintf(stderr, "usage: dmmcs_main absorb OUT N_PARTS [STATE PLANES N_ROWS G STRIDE CUR]...\n"
                    "       dmmcs_main rows OUT N H0 INDICES N_PARTS [PLANES N_ROWS COLS STRIDE]...\n");
    return 2;
}

// the file holds exactly `bytes` bytes: into p
static bool slurp(const char *path, uint8_t *p, size_t bytes) {
    FILE *f = fopen(path, "rb");
    if (f == nullptr) return false;
    const size_t got = fread(p, 1, bytes, f);
    const bool more = fgetc(f) != EOF;
    fclose(f);
    if (got != bytes || more) fprintf(stderr, "dmmcs_main: %s does not hold exactly %zu bytes\n", path, bytes);
    return got == bytes && !more;
}

static bool dump(const std::string &path, const uint8_t *p, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (f == nullptr) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

static uint8_t *block(size_t bytes) {
    void *p = nullptr;
    return posix_memalign(&p, 16, bytes) == 0 ? (uint8_t *)p : nullptr;
}

// the planes of a part, exactly ((g - 1) * stride + n_rows) * 32 bytes, the rows n_rows .. stride - 1 of every plane poisoned
static uint8_t *planes_of(const char *path, size_t n_rows, size_t g, size_t stride, bool poison) {
    const size_t bytes = ((g - 1) * stride + n_rows) * 32;
    uint8_t *d = block(bytes);
    if (d == nullptr || !slurp(path, d, bytes)) return nullptr;
    for (size_t c = 0; c + 1 < g; c++) {
        if (poison)
            DMMCS_POISON(d + (c * stride + n_rows) * 32, (stride - n_rows) * 32);
        else
            DMMCS_UNPOISON(d + (c * stride + n_rows) * 32, (stride - n_rows) * 32);
    }
    return d;
}

static int run_absorb(int argc, char **argv) {
    if (argc < 4) return usage();
    const std::string out = argv[2];
    const int n_live = atoi(argv[3]);
    if (n_live < 1 || n_live > HADES252_MMCS_MAX_GROUPS || argc != 4 + 6 * n_live) return usage();
    DmmcsParts table = {};
    uint8_t *planes[HADES252_MMCS_MAX_GROUPS], *state[HADES252_MMCS_MAX_GROUPS];
    uint64_t n_blocks = 0;
    for (int i = 0; i < n_live; i++) {
        char **a = argv + 4 + 6 * i;
        const size_t n_rows = (size_t)strtoull(a[2], nullptr, 0), g = (size_t)strtoull(a[3], nullptr, 0);
        const size_t stride = (size_t)strtoull(a[4], nullptr, 0), cur = (size_t)strtoull(a[5], nullptr, 0);
        if (n_rows == 0 || g == 0 || stride < n_rows || cur > 3) return usage();
        state[i] = block(n_rows * 160);
        if (state[i] == nullptr || !slurp(a[0], state[i], n_rows * 160)) return 3;
        planes[i] = planes_of(a[1], n_rows, g, stride, true);
        if (planes[i] == nullptr) return 3;
        table.planes[i] = planes[i];
        table.state[i] = state[i];
        table.S[i] = n_rows;
        table.stride[i] = stride;
        table.g[i] = g;
        table.first_block[i] = (uint32_t)n_blocks;
        table.cur[i] = (uint32_t)cur;
        n_blocks += (unsigned)((n_rows + kBlock - 1) / kBlock);
    }
    void *stream = nullptr;
    hipLaunchKernelGGL(k_dmmcs_absorb, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (uint32_t)n_live);
    for (int i = 0; i < n_live; i++) {
        if (!dump(out + ".state." + std::to_string(i), state[i], (size_t)table.S[i] * 160)) return 4;
        for (size_t c = 0; c + 1 < table.g[i]; c++)
            DMMCS_UNPOISON(planes[i] + (c * table.stride[i] + table.S[i]) * 32, (table.stride[i] - table.S[i]) * 32);
        free(planes[i]);
        free(state[i]);
    }
    return 0;
}

static int run_rows(int argc, char **argv) {
    if (argc < 7) return usage();
    const size_t n_queries = (size_t)strtoull(argv[3], nullptr, 0);
    const uint64_t h0 = strtoull(argv[4], nullptr, 0);
    const size_t n_parts = (size_t)strtoull(argv[6], nullptr, 0);
    if (n_queries == 0 || h0 == 0 || n_parts < 1 || n_parts > HADES252_MMCS_MAX_GROUPS || argc != 7 + 4 * (int)n_parts) return usage();
    uint8_t *idx = block(n_queries * 8);
    if (idx == nullptr || !slurp(argv[5], idx, n_queries * 8)) return 3;
    DmmcsRowParts table = {};
    uint8_t *planes[HADES252_MMCS_MAX_GROUPS];
    size_t rows_of[HADES252_MMCS_MAX_GROUPS];
    size_t row_cols = 0;
    uint64_t n_blocks = 0;
    for (size_t p = 0; p < n_parts; p++) {
        char **a = argv + 7 + 4 * p;
        const size_t n_rows = (size_t)strtoull(a[1], nullptr, 0), cols = (size_t)strtoull(a[2], nullptr, 0);
        const size_t stride = (size_t)strtoull(a[3], nullptr, 0);
        if (n_rows == 0 || cols == 0 || stride < n_rows || h0 % n_rows != 0) return usage();
        planes[p] = planes_of(a[0], n_rows, cols, stride, true);
        if (planes[p] == nullptr) return 3;
        rows_of[p] = n_rows;
        table.planes[p] = planes[p];
        table.stride[p] = stride;
        table.col_off[p] = row_cols;
        table.cols[p] = (uint32_t)cols;
        table.div[p] = (uint32_t)(h0 / n_rows);
        table.first_block[p] = (uint32_t)n_blocks;
        row_cols += cols;
        n_blocks += (unsigned)((n_queries * cols + kBlock - 1) / kBlock);
    }
    uint8_t *d_rows = block(n_queries * row_cols * 32);
    if (d_rows == nullptr) return 3;
    memset(d_rows, 0xA5, n_queries * row_cols * 32);
    const uint64_t *d_indices = (const uint64_t *)idx;
    void *stream = nullptr;
    hipLaunchKernelGGL(k_dmmcs_rows, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (uint32_t)n_parts, d_indices,
                       n_queries, (uint64_t)h0, row_cols, (uint8_t *)d_rows);
    if (!dump(argv[2], d_rows, n_queries * row_cols * 32)) return 4;
    for (size_t p = 0; p < n_parts; p++) {
        for (size_t c = 0; c + 1 < table.cols[p]; c++)
            DMMCS_UNPOISON(planes[p] + (c * table.stride[p] + rows_of[p]) * 32, (table.stride[p] - rows_of[p]) * 32);
        free(planes[p]);
    }
    free(d_rows);
    free(idx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return usage();
    const std::string what = argv[1];
    const int rc = what == "absorb" ? run_absorb(argc, argv) : what == "rows" ? run_rows(argc, argv) : usage();
    free(hostsim::g_lds_arena);
    hostsim::g_lds_arena = nullptr;
    return rc;
}
