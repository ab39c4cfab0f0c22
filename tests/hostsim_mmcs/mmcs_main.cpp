// mmcs_main.cpp -- the shipped kernels of hades252_amd/csrc/kernels_mmcs.hpp as a host program, for the CPU-tier test
// tests/test_mmcs_cpu_run.py (built with ASan + UBSan and run as an ordinary child process).
//
// <hip/hip_runtime.h> resolves to the stand-in of tests/hostsim (block emulator: see there); the tree's headers are the
// copies tests/hostsim_lib.py makes (rewritten(): the empty fences and the dynamic LDS declaration, nothing else).  Nothing
// in this file does arithmetic or defines a kernel or a device routine: it reads its inputs, launches k_mmcs_inject or
// k_mmcs_verify with the geometry of its call site in host_mmcs.hpp and writes what the kernel wrote.  Every buffer is a heap
// block of exactly its size: the nodes and the leaves of an injection (N * 32 bytes each), the indices (N * 8) and the roots
// (N * 32) of a verification; its rows and paths share one block with a poisoned gap of 64 bytes between them, so a row word
// read past the last row, a sibling read before the first path or past the last one, and a store past the last node or root
// is an ASan report.
//
//   mmcs_main inject OUT N OUT_IDX TAG0..3 NODES LEAVES
//   mmcs_main verify OUT N ARITY PAD_MODE OUT_IDX N_PERMS CAP0..3 TAG0..3 INJECT0..3 ROWS INDICES PATHS G COLS CLIMB [COLS CLIMB]...
//   (a scalar's four limbs; the group table as the host passes it: columns and levels to climb, tallest group first)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define MMCS_POISON(p, n) __asan_poison_memory_region((p), (n))
#define MMCS_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef MMCS_POISON
#define MMCS_POISON(p, n) ((void)0)
#define MMCS_UNPOISON(p, n) ((void)0)
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
#include "hades252_amd/csrc/kernels_mmcs.hpp"

static const size_t kGap = 64;

static int usage() {
    fprintf(stderr, "usage: mmcs_main inject OUT N OUT_IDX TAG0..3 NODES LEAVES\n"
                    "       mmcs_main verify OUT N ARITY PAD_MODE OUT_IDX N_PERMS CAP0..3 TAG0..3 INJECT0..3 ROWS INDICES PATHS G "
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
    if (got != bytes || more) fprintf(stderr, "mmcs_main: %s does not hold exactly %zu bytes\n", path, bytes);
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

static int run_inject(int argc, char **argv) {
    if (argc != 11) return usage();
    const size_t n = (size_t)strtoull(argv[3], nullptr, 0);
    const int out_idx = atoi(argv[4]);
    const Fr inject_tag = scalar(argv + 5);
    if (n == 0) return usage();
    uint8_t *nodes = block(n * 32), *leaf = block(n * 32);
    if (nodes == nullptr || leaf == nullptr || !slurp(argv[9], nodes, n * 32) || !slurp(argv[10], leaf, n * 32)) return 3;
    hipLaunchKernelGGL(k_mmcs_inject, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t) nullptr, nodes, leaf, n,
                       inject_tag, out_idx);
    if (!dump(argv[2], nodes, n * 32)) return 4;
    free(nodes);
    free(leaf);
    return 0;
}

static int run_verify(int argc, char **argv) {
    if (argc < 25) return usage();
    const size_t m = (size_t)strtoull(argv[3], nullptr, 0);
    const int arity = atoi(argv[4]), pad_mode = atoi(argv[5]), out_idx = atoi(argv[6]);
    const size_t n_perms = (size_t)strtoull(argv[7], nullptr, 0);
    const Fr cap = scalar(argv + 8), tag = scalar(argv + 12), inject_tag = scalar(argv + 16);
    const uint32_t n_groups = (uint32_t)strtoul(argv[23], nullptr, 0);
    if (m == 0 || arity < 2 || arity > 4 || n_groups < 1 || n_groups > HADES252_MMCS_MAX_GROUPS || argc != 24 + 2 * (int)n_groups)
        return usage();
    MmcsGroups table = {};
    size_t row_cols = 0;
    uint32_t depth = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
        table.cols[g] = (uint32_t)strtoul(argv[24 + 2 * g], nullptr, 0);
        table.climb[g] = (uint32_t)strtoul(argv[25 + 2 * g], nullptr, 0);
        row_cols += table.cols[g];
        depth += table.climb[g];
    }
    const size_t rows_b = m * row_cols * 32, paths_b = m * (size_t)depth * (arity - 1) * 32;
    uint8_t *both = block(rows_b + kGap + paths_b), *idx = block(m * 8), *d_roots = block(m * 32);
    if (both == nullptr || idx == nullptr || d_roots == nullptr) return 3;
    uint8_t *d_rows = both, *d_paths = both + rows_b + kGap;
    if (!slurp(argv[20], d_rows, rows_b) || !slurp(argv[21], idx, m * 8) || !slurp(argv[22], d_paths, paths_b)) return 3;
    memset(d_roots, 0xA5, m * 32);
    MMCS_POISON(both + rows_b, kGap);
    const uint64_t *d_idx = (const uint64_t *)idx;
    hipStream_t s = nullptr;
#define HADES_LAUNCH_MMCS_VERIFY(A)                                                                                        \
    hipLaunchKernelGGL(k_mmcs_verify<A>, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_rows, d_idx, d_paths, m, table, n_groups, \
                       row_cols, depth, n_perms, pad_mode, cap, tag, inject_tag, out_idx, d_roots)
    switch (arity) {
        case 2: HADES_LAUNCH_MMCS_VERIFY(2); break;
        case 3: HADES_LAUNCH_MMCS_VERIFY(3); break;
        default: HADES_LAUNCH_MMCS_VERIFY(4); break;
    }
#undef HADES_LAUNCH_MMCS_VERIFY
    MMCS_UNPOISON(both + rows_b, kGap);
    if (!dump(argv[2], d_roots, m * 32)) return 4;
    free(both);
    free(idx);
    free(d_roots);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return usage();
    const std::string what = argv[1];
    const int rc = what == "inject" ? run_inject(argc, argv) : what == "verify" ? run_verify(argc, argv) : usage();
    free(hostsim::g_lds_arena);
    hostsim::g_lds_arena = nullptr;
    return rc;
}
