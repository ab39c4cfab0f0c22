// inverse_main.cpp -- the shipped kernels of hades252_amd/csrc/kernels_inverse.hpp as a host program, for the CPU-tier test
// tests/test_inverse_cpu_run.py (built with ASan + UBSan and run as an ordinary child process).
//
// <hip/hip_runtime.h> resolves to the stand-in of tests/hostsim (block emulator: see there); the tree's headers are the
// copies tests/hostsim_lib.py makes (rewritten(): the empty fences and the dynamic LDS declaration, nothing else).  Nothing
// in this file does arithmetic or defines a kernel or a device routine: it reads a buffer, launches ONE shipped kernel with
// the geometry of its call site in host_inverse.hpp on a heap block of exactly the data's size, and writes the buffer back.
//
//   inverse_main rounds IN OUT N ROUND_HI ROUND_LO     N states of 160 bytes
//   inverse_main root   IN OUT N                       N scalars of 32 bytes
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
#include "hades252_amd/csrc/hades_inverse_constants.inc"
#include "hades252_amd/csrc/kernels_inverse.hpp"

static int usage() {
    fprintf(stderr, "usage: inverse_main rounds IN OUT N ROUND_HI ROUND_LO | inverse_main root IN OUT N\n");
    return 2;
}

int main(int argc, char **argv) {
    if (argc < 5) return usage();
    const bool root = strcmp(argv[1], "root") == 0;
    if (!root && (strcmp(argv[1], "rounds") != 0 || argc != 7)) return usage();
    const size_t n = (size_t)strtoull(argv[4], nullptr, 0), bytes = n * (root ? 32 : 160);
    FILE *f = fopen(argv[2], "rb");
    if (f == nullptr) return usage();
    uint8_t *buf = nullptr;
    if (posix_memalign((void **)&buf, 16, bytes) != 0) return 3;       // exactly the data: ASan sees byte `bytes`
    const size_t got = fread(buf, 1, bytes, f);
    const bool more = fgetc(f) != EOF;
    fclose(f);
    if (got != bytes || more) {
        fprintf(stderr, "inverse_main: %s does not hold exactly %zu bytes\n", argv[2], bytes);
        return 3;
    }
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    if (root) {
        hipLaunchKernelGGL(k_fifth_root, grid, block, 0, (hipStream_t) nullptr, buf, n);
    } else {
        const int hi = atoi(argv[5]), lo = atoi(argv[6]);
        if (lo < 0 || lo >= hi || hi > HADES252_ROUNDS_TOTAL) return usage();
        hipLaunchKernelGGL(k_perm_inverse, grid, block, (size_t)kWavesPerBlock * lds_wave_bytes(5), (hipStream_t) nullptr, buf, n,
                           hi, lo);
    }
    f = fopen(argv[3], "wb");
    if (f == nullptr || fwrite(buf, 1, bytes, f) != bytes) return 4;
    fclose(f);
    free(buf);
    free(hostsim::g_lds_arena);
    hostsim::g_lds_arena = nullptr;
    return 0;
}
