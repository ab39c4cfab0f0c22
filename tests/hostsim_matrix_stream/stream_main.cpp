// stream_main.cpp -- the shipped kernels of hades252_amd/csrc/kernels_matrix_stream.hpp as a host program, for the CPU-tier
// test tests/test_matrix_stream_cpu_run.py (built with ASan + UBSan and run as an ordinary child process).
//
// <hip/hip_runtime.h> resolves to the stand-in of tests/hostsim (block emulator: see there); the tree's headers are the
// copies tests/hostsim_lib.py makes (rewritten(): the empty fences and the dynamic LDS declaration, nothing else).  Nothing
// in this file does arithmetic or defines a kernel or a device routine: it opens a fresh state (k_planes_init), absorbs one
// group of columns after the other (k_planes_absorb, one tile per group) and finishes (k_planes_finish), each with the
// geometry of its call site in host_matrix_stream.hpp, and writes the state planes after every absorb, the digests, and the
// state planes once more after the finish.  The state planes are a heap block of exactly N_ROWS * 160 bytes and the digests
// one of exactly N_ROWS * 32 bytes; the planes of a group are a heap block of exactly ((G - 1) * STRIDE + N_ROWS) * 32 bytes
// -- the last plane ends with its last row -- and the gap between two planes (rows N_ROWS .. STRIDE - 1) is poisoned, so an
// access past ANY plane's last row is an ASan report.
//
//   stream_main OUT N_ROWS PAD_MODE CAP0 CAP1 CAP2 CAP3 [PLANES G STRIDE]...       (the capacity's four limbs; one triple
//                                                                                  per group)
//   writes OUT.state.<i> after group i (from 0), OUT.digests, OUT.state.end
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define STREAM_POISON(p, n) __asan_poison_memory_region((p), (n))
#define STREAM_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef STREAM_POISON
#define STREAM_POISON(p, n) ((void)0)
#define STREAM_UNPOISON(p, n) ((void)0)
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
#include "hades252_amd/csrc/kernels_matrix_stream.hpp"

static int usage() {
    fprintf(stderr, "usage: stream_main OUT N_ROWS PAD_MODE CAP0 CAP1 CAP2 CAP3 [PLANES G STRIDE]...\n");
    return 2;
}

static bool dump(const std::string &path, const uint8_t *p, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (f == nullptr) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
    if (argc < 8 || (argc - 8) % 3 != 0) return usage();
    const std::string out = argv[1];
    const size_t n_rows = (size_t)strtoull(argv[2], nullptr, 0);
    const int pad_mode = atoi(argv[3]);
    if (n_rows == 0 || (pad_mode != 0 && pad_mode != 1)) return usage();
    Fr cap;
    for (int k = 0; k < 4; k++) {
        const uint64_t v = strtoull(argv[4 + k], nullptr, 0);
        cap.l[2 * k] = (uint32_t)v;
        cap.l[2 * k + 1] = (uint32_t)(v >> 32);
    }
    const size_t S = n_rows, m = n_rows, state_bytes = n_rows * 160, out_bytes = n_rows * 32;
    uint8_t *state = nullptr, *digests = nullptr;
    if (posix_memalign((void **)&state, 16, state_bytes) != 0 || posix_memalign((void **)&digests, 16, out_bytes) != 0) return 3;
    memset(state, 0x5A, state_bytes);
    memset(digests, 0xA5, out_bytes);
    hipLaunchKernelGGL(k_planes_init, dim3((unsigned)((n_rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t) nullptr, state,
                       n_rows, n_rows, cap);
    uint64_t total = 0;
    for (int a = 8, i = 0; a < argc; a += 3, i++) {
        const size_t gw = (size_t)strtoull(argv[a + 1], nullptr, 0), K = (size_t)strtoull(argv[a + 2], nullptr, 0);
        if (gw == 0 || K < n_rows) return usage();
        const size_t bytes = ((gw - 1) * K + n_rows) * 32;
        FILE *f = fopen(argv[a], "rb");
        uint8_t *d = nullptr;
        if (f == nullptr || posix_memalign((void **)&d, 16, bytes) != 0) return 3;
        const size_t got = fread(d, 1, bytes, f);
        const bool more = fgetc(f) != EOF;
        fclose(f);
        if (got != bytes || more) {
            fprintf(stderr, "stream_main: %s does not hold exactly %zu bytes\n", argv[a], bytes);
            return 3;
        }
        for (size_t c = 0; c + 1 < gw; c++) STREAM_POISON(d + (c * K + n_rows) * 32, (K - n_rows) * 32);
        const unsigned cur = (unsigned)(total % 4);
        hipLaunchKernelGGL(k_planes_absorb, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t) nullptr, state,
                           S, m, d, gw, K, (int)cur);
        for (size_t c = 0; c + 1 < gw; c++) STREAM_UNPOISON(d + (c * K + n_rows) * 32, (K - n_rows) * 32);
        free(d);
        total += gw;
        if (!dump(out + ".state." + std::to_string(i), state, state_bytes)) return 4;
    }
    if (total != 0) {
        hipLaunchKernelGGL(k_planes_finish, dim3((unsigned)((S + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t) nullptr, state,
                           S, S, digests, (int)(total % 4), pad_mode);
        if (!dump(out + ".digests", digests, out_bytes) || !dump(out + ".state.end", state, state_bytes)) return 4;
    }
    free(state);
    free(digests);
    free(hostsim::g_lds_arena);
    hostsim::g_lds_arena = nullptr;
    return 0;
}
