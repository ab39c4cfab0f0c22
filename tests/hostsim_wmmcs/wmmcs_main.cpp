// wmmcs_main.cpp -- the shipped kernel of hades252_amd/csrc/kernels_wmmcs.hpp as a host program, for the CPU-tier test
// tests/test_wmmcs_cpu_run.py (built with ASan + UBSan and run as an ordinary child process).
//
// <hip/hip_runtime.h> resolves to the stand-in of tests/hostsim (block emulator: see there); the tree's headers are the
// copies tests/hostsim_lib.py makes (rewritten(): the empty fences and the dynamic LDS declaration, nothing else).  Nothing
// in this file does arithmetic or defines a kernel or a device routine: it reads its inputs, launches k_mmcs_inputs with the
// geometry of its call site in abi_wmmcs.hpp and writes what the kernel wrote.  Every buffer is a heap block of exactly its
// size: the rows (N * ROW_COLS * 32 bytes), the indices (N * 8), the paths (N * DEPTH * (ARITY - 1) * 32), the inputs
// (N_PERMS * N * 160) and the roots (N * 32, or none at all), so a row word past the last row, a sibling outside the paths, a
// state word past the last record or a root past the last query is an ASan report.
//
//   wmmcs_main OUT N ARITY PAD_MODE OUT_IDX N_PERMS CAP0..3 TAG0..3 INJECT0..3 ROWS INDICES PATHS WANT_ROOTS G COLS CLIMB [COLS CLIMB]...
//   (a scalar's four limbs; the group table as the host passes it: columns and levels to climb, tallest group first;
//   WANT_ROOTS 0: d_roots = NULL).  Writes OUT (the inputs) and, with roots, OUT.roots.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

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
#include "hades252_amd/csrc/kernels_mmcs.hpp"
#include "hades252_amd/csrc/kernels_wmmcs.hpp"

static int usage() {
    fprintf(stderr, "usage: wmmcs_main OUT N ARITY PAD_MODE OUT_IDX N_PERMS CAP0..3 TAG0..3 INJECT0..3 ROWS INDICES PATHS WANT_ROOTS G "
                    "COLS CLIMB [COLS CLIMB]...\n");
    return 2;
}

static Fr scalar(char **argv) {
    Fr r;
    for (int k = 0; k < 4; k++) {
        const uint64_t v = strtoull(argv[k], nullptr, 0);
        r.l[2 * k] = (uint32_t)v;
        r.l[2 * k + 1] = (uint32_t)(v >> 32);
    }
    return r;
}

// the file holds exactly `bytes` bytes: into p
static bool slurp(const char *path, uint8_t *p, size_t bytes) {
    FILE *f = fopen(path, "rb");
    if (f == nullptr) return false;
    const size_t got = fread(p, 1, bytes, f);
    const bool more = fgetc(f) != EOF;
    fclose(f);
    if (got != bytes || more) fprintf(stderr, "wmmcs_main: %s does not hold exactly %zu bytes\n", path, bytes);
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

static int run(int argc, char **argv) {
    if (argc < 26) return usage();
    const std::string out = argv[1];
    const size_t n_queries = (size_t)strtoull(argv[2], nullptr, 0);
    const int arity = atoi(argv[3]), pad_mode = atoi(argv[4]), out_idx = atoi(argv[5]);
    const size_t n_perms = (size_t)strtoull(argv[6], nullptr, 0);
    const Fr cap = scalar(argv + 7), tag = scalar(argv + 11), inject_tag = scalar(argv + 15);
    const bool want_roots = atoi(argv[22]) != 0;
    const size_t n_groups = (size_t)strtoull(argv[23], nullptr, 0);
    if (n_queries == 0 || n_perms == 0 || arity < 2 || arity > 4 || n_groups < 1 || n_groups > HADES252_MMCS_MAX_GROUPS ||
        argc != 24 + 2 * (int)n_groups)
        return usage();
    MmcsGroups table = {};
    size_t row_cols = 0;
    uint32_t depth = 0;
    for (size_t g = 0; g < n_groups; g++) {
        table.cols[g] = (uint32_t)strtoul(argv[24 + 2 * g], nullptr, 0);
        table.climb[g] = (uint32_t)strtoul(argv[25 + 2 * g], nullptr, 0);
        row_cols += table.cols[g];
        depth += table.climb[g];
    }
    const size_t rows_b = n_queries * row_cols * 32, paths_b = n_queries * (size_t)depth * (arity - 1) * 32;
    const size_t inputs_b = n_perms * n_queries * 160;
    uint8_t *d_rows = block(rows_b), *idx = block(n_queries * 8), *d_paths = block(paths_b), *d_inputs = block(inputs_b);
    uint8_t *d_roots = want_roots ? block(n_queries * 32) : nullptr;
    if (d_rows == nullptr || idx == nullptr || d_paths == nullptr || d_inputs == nullptr || (want_roots && d_roots == nullptr)) return 3;
    if (!slurp(argv[19], d_rows, rows_b) || !slurp(argv[20], idx, n_queries * 8) || !slurp(argv[21], d_paths, paths_b)) return 3;
    memset(d_inputs, 0xA5, inputs_b);
    if (want_roots) memset(d_roots, 0xA5, n_queries * 32);
    const uint64_t *d_idx = (const uint64_t *)idx;
    hipStream_t s = nullptr;
#define HADES_LAUNCH_MMCS_INPUTS(A)                                                                                                   \
    hipLaunchKernelGGL(k_mmcs_inputs<A>, dim3((unsigned)((n_queries + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (const uint8_t *)d_rows, \
                       d_idx, (const uint8_t *)d_paths, n_queries, table, (uint32_t)n_groups, row_cols, depth, n_perms, pad_mode, cap,   \
                       tag, inject_tag, out_idx, (uint8_t *)d_inputs, (uint8_t *)d_roots)
    switch (arity) {
        case 2: HADES_LAUNCH_MMCS_INPUTS(2); break;
        case 3: HADES_LAUNCH_MMCS_INPUTS(3); break;
        default: HADES_LAUNCH_MMCS_INPUTS(4); break;
    }
#undef HADES_LAUNCH_MMCS_INPUTS
    if (!dump(out, d_inputs, inputs_b) || (want_roots && !dump(out + ".roots", d_roots, n_queries * 32))) return 4;
    free(d_rows);
    free(idx);
    free(d_paths);
    free(d_inputs);
    free(d_roots);
    return 0;
}

int main(int argc, char **argv) {
    const int rc = run(argc, argv);
    free(hostsim::g_lds_arena);
    hostsim::g_lds_arena = nullptr;
    return rc;
}
