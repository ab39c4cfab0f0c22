// rowmajor_main.cpp -- the shipped kernels of hades252_amd/csrc/kernels_rowmajor.hpp as a host program, for the CPU-tier test
// tests/test_rowmajor_cpu_run.py (built with ASan + UBSan and run as an ordinary child process).
//
// <hip/hip_runtime.h> resolves to the stand-in of tests/hostsim (block emulator: see there); the tree's headers are the
// copies tests/hostsim_lib.py makes (rewritten(): the empty fences and the dynamic LDS declaration, nothing else).  Nothing
// in this file does arithmetic or defines a kernel or a device routine: it reads its inputs, fills the part table the way
// abi_rowmajor.hpp does (the blocks of all parts laid end to end, in the order given; the two steps of a part from its
// layout), launches k_rm_absorb or k_rm_rows with the geometry of its call site there and writes what the kernel wrote.
// Every buffer is a heap block of exactly its size: the five state planes of a part (N_ROWS * 160 bytes), the indices
// (N * 8) and the output rows (N * ROW_COLS * 32).  A matrix ends with its last scalar -- row-major (LAYOUT 1):
// ((N_ROWS - 1) * STRIDE + G) * 32 bytes, the last row ends with its last column; column-major (LAYOUT 0):
// ((G - 1) * STRIDE + N_ROWS) * 32 bytes -- and the gap behind every row (every plane) but the last is poisoned, so a read
// past ANY row's width or plane's height, any state plane, the last index or the last output scalar is an ASan report.
//
//   rowmajor_main absorb OUT N_PARTS [STATE MAT N_ROWS G STRIDE CUR LAYOUT]...   writes OUT.state.<p>: part p's state planes after
//   rowmajor_main rows OUT N H0 INDICES N_PARTS [MAT N_ROWS COLS STRIDE LAYOUT]... writes OUT: N x (sum of COLS) scalars
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define RM_POISON(p, n) __asan_poison_memory_region((p), (n))
#define RM_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef RM_POISON
#define RM_POISON(p, n) ((void)0)
#define RM_UNPOISON(p, n) ((void)0)
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
#include "hades252_amd/csrc/kernels_rowmajor.hpp"

static int usage() {
    fprintf(stderr, "usage: rowmajor_main absorb OUT N_PARTS [STATE MAT N_ROWS G STRIDE CUR LAYOUT]...\n"
                    "       rowmajor_main rows OUT N H0 INDICES N_PARTS [MAT N_ROWS COLS STRIDE LAYOUT]...\n");
    return 2;
}

// the file holds exactly `bytes` bytes: into p
static bool slurp(const char *path, uint8_t *p, size_t bytes) {
    FILE *f = fopen(path, "rb");
    if (f == nullptr) return false;
    const size_t got = fread(p, 1, bytes, f);
    const bool more = fgetc(f) != EOF;
    fclose(f);
    if (got != bytes || more) fprintf(stderr, "rowmajor_main: %s does not hold exactly %zu bytes\n", path, bytes);
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

// A matrix as its layout strides it: `runs` runs of `len` scalars, `stride` scalars apart (row-major: the rows, g long;
// column-major: the planes, n_rows long).
struct Mat {
    uint8_t *d = nullptr;
    size_t runs = 0, len = 0, stride = 0;
    uint64_t row_step = 0, col_step = 0;
};

// the gaps behind every run but the last: poisoned while the kernel runs
static void gaps(const Mat &m, bool poison) {
    for (size_t r = 0; r + 1 < m.runs; r++) {
        if (poison)
            RM_POISON(m.d + (r * m.stride + m.len) * 32, (m.stride - m.len) * 32);
        else
            RM_UNPOISON(m.d + (r * m.stride + m.len) * 32, (m.stride - m.len) * 32);
    }
}

// the matrix of a part, exactly up to its last scalar, and its two steps (rm_steps of abi_rowmajor.hpp)
static bool mat_of(const char *path, size_t n_rows, size_t g, size_t stride, unsigned layout, Mat &m) {
    if (layout == HADES252_LAYOUT_COLS) {
        if (stride < n_rows) return false;
        m.runs = g, m.len = n_rows;
        m.row_step = 1;
        m.col_step = stride;
    } else {
        if (layout != HADES252_LAYOUT_ROWS || stride < g) return false;
        m.runs = n_rows, m.len = g;
        m.row_step = stride;
        m.col_step = 1;
    }
    m.stride = stride;
    const size_t bytes = ((m.runs - 1) * stride + m.len) * 32;
    m.d = block(bytes);
    if (m.d == nullptr || !slurp(path, m.d, bytes)) return false;
    gaps(m, true);
    return true;
}

static void mat_free(Mat &m) {
    gaps(m, false);
    free(m.d);
    m.d = nullptr;
}

static int run_absorb(int argc, char **argv) {
    if (argc < 4) return usage();
    const std::string out = argv[2];
    const int n_live = atoi(argv[3]);
    if (n_live < 1 || n_live > HADES252_MMCS_MAX_GROUPS || argc != 4 + 7 * n_live) return usage();
    RmParts table = {};
    Mat mats[HADES252_MMCS_MAX_GROUPS];
    uint8_t *state[HADES252_MMCS_MAX_GROUPS];
    uint64_t n_blocks = 0;
    for (int i = 0; i < n_live; i++) {
        char **a = argv + 4 + 7 * i;
        const size_t n_rows = (size_t)strtoull(a[2], nullptr, 0), g = (size_t)strtoull(a[3], nullptr, 0);
        const size_t stride = (size_t)strtoull(a[4], nullptr, 0), cur = (size_t)strtoull(a[5], nullptr, 0);
        if (n_rows == 0 || g == 0 || cur > 3) return usage();
        state[i] = block(n_rows * 160);
        if (state[i] == nullptr || !slurp(a[0], state[i], n_rows * 160)) return 3;
        if (!mat_of(a[1], n_rows, g, stride, (unsigned)strtoul(a[6], nullptr, 0), mats[i])) return 3;
        table.base[i] = mats[i].d;
        table.state[i] = state[i];
        table.S[i] = n_rows;
        table.rows[i] = n_rows;
        table.row_step[i] = mats[i].row_step;
        table.col_step[i] = mats[i].col_step;
        table.g[i] = g;
        table.first_block[i] = (uint32_t)n_blocks;
        table.cur[i] = (uint32_t)cur;
        n_blocks += (unsigned)((n_rows + kBlock - 1) / kBlock);
    }
    void *stream = nullptr;
    hipLaunchKernelGGL(k_rm_absorb, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (uint32_t)n_live);
    for (int i = 0; i < n_live; i++) {
        if (!dump(out + ".state." + std::to_string(i), state[i], (size_t)table.S[i] * 160)) return 4;
        mat_free(mats[i]);
        free(state[i]);
    }
    return 0;
}

static int run_rows(int argc, char **argv) {
    if (argc < 7) return usage();
    const size_t n_queries = (size_t)strtoull(argv[3], nullptr, 0);
    const uint64_t h0 = strtoull(argv[4], nullptr, 0);
    const size_t n_parts = (size_t)strtoull(argv[6], nullptr, 0);
    if (n_queries == 0 || h0 == 0 || n_parts < 1 || n_parts > HADES252_MMCS_MAX_GROUPS || argc != 7 + 5 * (int)n_parts) return usage();
    uint8_t *idx = block(n_queries * 8);
    if (idx == nullptr || !slurp(argv[5], idx, n_queries * 8)) return 3;
    RmRowParts table = {};
    Mat mats[HADES252_MMCS_MAX_GROUPS];
    size_t row_cols = 0;
    uint64_t n_blocks = 0;
    for (size_t p = 0; p < n_parts; p++) {
        char **a = argv + 7 + 5 * p;
        const size_t n_rows = (size_t)strtoull(a[1], nullptr, 0), cols = (size_t)strtoull(a[2], nullptr, 0);
        const size_t stride = (size_t)strtoull(a[3], nullptr, 0);
        if (n_rows == 0 || cols == 0 || h0 % n_rows != 0) return usage();
        if (!mat_of(a[0], n_rows, cols, stride, (unsigned)strtoul(a[4], nullptr, 0), mats[p])) return 3;
        table.base[p] = mats[p].d;
        table.row_step[p] = mats[p].row_step;
        table.col_step[p] = mats[p].col_step;
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
    hipLaunchKernelGGL(k_rm_rows, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (uint32_t)n_parts, d_indices,
                       n_queries, (uint64_t)h0, row_cols, (uint8_t *)d_rows);
    if (!dump(argv[2], d_rows, n_queries * row_cols * 32)) return 4;
    for (size_t p = 0; p < n_parts; p++) mat_free(mats[p]);
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
