// hostsim_main.cpp -- the shipped device sources, launch policy and device-pointer C ABI of hades252_amd/csrc as ONE host
// program, for the CPU-tier tests tests/test_hostsim_*.py (built by tests/hostsim_lib.py with ASan+UBSan, and with TSan).
//
// The include list is that of hades252_amd/csrc/hades252.hip without the host plumbing (host_pin / host_pool / host_pipe /
// host_callers / host_safe / host_cipher); host_fault.hpp stays because the abi_*.hpp files use its HIP_TRY and fault hook.
// <hip/hip_runtime.h> resolves to the stand-in in this directory (block emulator: see there).  The unit kernels of
// tests/units/arith_units.hip come along unchanged.  Nothing in this file does arithmetic or defines a kernel: it is a
// table of entry points and a script reader.
//
// Script (stdin), one command per line:
//   buf NAME file PATH        NAME = the bytes of PATH, in a heap block of EXACTLY that size (ASan sees byte n)
//   buf NAME zero BYTES       ... or BYTES zero bytes
//   buf NAME fill BYTES V     ... or BYTES bytes of value V
//   call FUNC ARG...          one argument per parameter: a pointer is NAME, NAME+OFFSET or null; an integer is parsed
//                             prints "rc FUNC VALUE"
//                             and, with HOSTSIM_SKIP_NOT_EMULATED=1, "not_emulated FUNC BUILTIN" when a launch met a DPP form
//   dump NAME PATH            the bytes of NAME -> PATH
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <pthread.h>
#include <sched.h>

#include <atomic>
#include <thread>
#include <vector>

// Entry points and kernels get internal linkage, so that a part build (HOSTSIM_PART below) emits code only for what its
// table names: the whole unit under the sanitizers takes minutes to compile, its four parts compile side by side.
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
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
#include "hades252_amd/csrc/kernels_perm.hpp"
#include "hades252_amd/csrc/kernels_merkle.hpp"
#include "hades252_amd/csrc/kernels_sponge.hpp"
#include "hades252_amd/csrc/kernels_cipher.hpp"
#include "hades252_amd/csrc/kernels_safe.hpp"
#include "hades252_amd/csrc/kernels_witness.hpp"
#include "hades252_amd/csrc/kernels_aux.hpp"

#include "hades252_amd/csrc/host_fault.hpp"
#include "hades252_amd/csrc/launch.hpp"
#include "hades252_amd/csrc/abi_perm.hpp"
#include "hades252_amd/csrc/abi_merkle.hpp"
#include "hades252_amd/csrc/abi_sponge.hpp"
#include "hades252_amd/csrc/abi_cipher.hpp"
#include "hades252_amd/csrc/abi_safe.hpp"
#include "hades252_amd/csrc/abi_witness.hpp"
#include "hades252_amd/csrc/abi_util.hpp"

#include "tests/units/arith_units.hip"
#pragma clang attribute pop

#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <type_traits>

namespace driver {

struct Buf {
    uint8_t *p;
    size_t n;
};
static std::map<std::string, Buf> g_bufs;

[[noreturn]] static void fail(const std::string &why) {
    fprintf(stderr, "hostsim driver: %s\n", why.c_str());
    exit(2);
}

static uint8_t *exact_block(size_t n) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1) != 0) fail("out of memory");       // 16-byte aligned, like device allocations
    return (uint8_t *)p;
}

// one argument, its kind taken from the parameter's own type
template <class T>
static T parse(const std::string &tok) {
    if constexpr (std::is_pointer_v<T>) {
        if (tok == "null") return nullptr;
        const size_t plus = tok.find('+');
        const std::string name = tok.substr(0, plus);
        const auto it = g_bufs.find(name);
        if (it == g_bufs.end()) fail("no buffer named " + name);
        const size_t off = plus == std::string::npos ? 0 : (size_t)strtoull(tok.c_str() + plus + 1, nullptr, 0);
        if (off > it->second.n) fail("offset past the end of " + name);
        return (T)(it->second.p + off);
    } else if constexpr (std::is_signed_v<T>) {
        return (T)strtoll(tok.c_str(), nullptr, 0);
    } else {
        return (T)strtoull(tok.c_str(), nullptr, 0);
    }
}

using Call = std::function<void(const std::vector<std::string> &)>;
static std::map<std::string, Call> g_table;

template <class R, class... A>
static void reg(const char *name, R (*fn)(A...)) {
    g_table[name] = [name, fn](const std::vector<std::string> &tok) {
        if (tok.size() != sizeof...(A)) fail(std::string(name) + ": wrong number of arguments");
        size_t i = 0;
        std::tuple<std::decay_t<A>...> args{parse<std::decay_t<A>>(tok[i++])...};      // braces: left to right
        (void)i;
        const R r = std::apply(fn, args);
        if (const char *what = hostsim::g_not_emulated.exchange(nullptr)) printf("not_emulated %s %s\n", name, what);
        if constexpr (std::is_pointer_v<R>)
            printf("rc %s %s\n", name, r ? (const char *)r : "(null)");
        else
            printf("rc %s %lld\n", name, (long long)r);
    };
}
#define REG(f) reg(#f, &f)

// which entry points this executable holds: bit 0 perm + units, 1 merkle, 2 sponge / cipher / duplex sponge / generators,
// 3 chain witnesses; all of them by default (one program, as hades252.hip is one library)
#ifndef HOSTSIM_PART
#define HOSTSIM_PART 15
#endif

static void register_all() {
#if HOSTSIM_PART & 1
    // abi_perm.hpp
    REG(hades252_rounds); REG(hades252_device_count); REG(hades252_strerror); REG(hades252_last_hip_error);
    REG(hades252_version); REG(hades252_perm_batch_dev_ex); REG(hades252_perm_batch_dev); REG(hades252_kernel_for);
    REG(hades252_chain_form_for); REG(hades252_kernel_name); REG(hades252_perm_trace_dev_ex); REG(hades252_witness_wires);
    REG(hades252_perm_witness_dev); REG(hades252_perm_trace_scaled_dev); REG(hades252_perm_trace_scale_table);
    REG(hades252_perm_trace_dev); REG(hades252_add_round_key_at_dev); REG(hades252_apply_full_round_at_dev);
    REG(hades252_apply_partial_round_at_dev); REG(hades252_add_round_key_dev); REG(hades252_apply_full_round_dev);
    REG(hades252_apply_partial_round_dev); REG(hades252_fr_op_dev); REG(hades252_mul_matrix_dev);
    REG(hades252_quintic_s_box_dev); REG(hades252_from_bytes_dev); REG(hades252_to_bytes_dev);
    // launch.hpp: the launcher the host-pointer path uses with out != in (no device-pointer entry point reaches that shape)
    REG(launch_perm_fast);
#endif
#if HOSTSIM_PART & 2
    // abi_merkle.hpp
    REG(hades252_merkle_depth); REG(hades252_merkle_level_pad_dev); REG(hades252_merkle_level_dev);
    REG(hades252_merkle4_level_dev); REG(hades252_merkle_tree_bytes); REG(hades252_merkle_scratch_bytes);
    REG(hades252_merkle4_scratch_bytes); REG(hades252_merkle_root_pad_dev); REG(hades252_merkle_root_dev);
    REG(hades252_merkle4_root_dev); REG(hades252_merkle_build_pad_dev); REG(hades252_merkle_build_dev);
    REG(hades252_merkle_update_dev); REG(hades252_merkle_empty_digests_dev); REG(hades252_merkle_open_pad_dev);
    REG(hades252_merkle_open_dev); REG(hades252_merkle_verify_dev); REG(hades252_merkle_forest_scratch_bytes);
    REG(hades252_merkle_forest_dev);
#endif
#if HOSTSIM_PART & 4
    // abi_sponge.hpp
    REG(hades252_sponge_hash_dev); REG(hades252_sponge_sort_scratch_bytes); REG(hades252_sponge_hash_var_ex_dev);
    REG(hades252_sponge_hash_var_dev); REG(hades252_sponge_init_dev); REG(hades252_sponge_absorb_dev);
    REG(hades252_sponge_squeeze_dev);
    // abi_cipher.hpp
    REG(hades252_cipher_encrypt_dev); REG(hades252_cipher_decrypt_dev);
    // abi_safe.hpp
    REG(hades252_safe_pattern); REG(hades252_safe_hash_dev); REG(hades252_safe_absorb_dev); REG(hades252_safe_squeeze_dev);
#endif
#if HOSTSIM_PART & 8
    // abi_witness.hpp
    REG(hades252_sponge_blocks); REG(hades252_sponge_witness_dev); REG(hades252_merkle_open_witness_dev);
    REG(hades252_cipher_perms); REG(hades252_cipher_encrypt_witness_dev); REG(hades252_cipher_decrypt_witness_dev);
    REG(hades252_safe_witness_dev); REG(hades252_safe_absorb_witness_dev); REG(hades252_safe_squeeze_witness_dev);
    // ... and what defines them: wires == hades252_perm_witness_dev(inputs); the states they run on come from the sponge
    REG(hades252_perm_witness_dev); REG(hades252_sponge_init_dev);
#endif
#if HOSTSIM_PART & 4
    // abi_util.hpp
    REG(hades252_gen_b_dev); REG(hades252_gen_a_dev); REG(hades252_digest_dev);
#endif
#if HOSTSIM_PART & 1
    // tests/units/arith_units.hip (the per-lane routines; the units_lane_* ones need DPP and are not emulated)
    REG(units_to_f29); REG(units_from_f29); REG(units_mont_mul); REG(units_mont_sqr); REG(units_mont_mul_const);
    REG(units_mont_mul_small); REG(units_mont_lin); REG(units_mont_lin1); REG(units_sbox29); REG(units_add_lazy);
    REG(units_small_mds); REG(units_finalize); REG(units_finalize1); REG(units_finalize32); REG(units_mds_row_cols);
    REG(units_fr_add); REG(units_fr_cond_sub_p); REG(units_fr_mul); REG(units_fr_is_canonical);
#endif
}

static std::vector<std::string> split(const std::string &line) {
    std::vector<std::string> out;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && isspace((unsigned char)line[i])) i++;
        size_t j = i;
        while (j < line.size() && !isspace((unsigned char)line[j])) j++;
        if (j > i) out.push_back(line.substr(i, j - i));
        i = j;
    }
    return out;
}

static int run(FILE *in) {
    register_all();
    char *lineptr = nullptr;
    size_t cap = 0;
    while (getline(&lineptr, &cap, in) >= 0) {
        std::vector<std::string> t = split(lineptr);
        if (t.empty() || t[0][0] == '#') continue;
        if (t[0] == "list") {
            for (const auto &kv : g_table) printf("entry %s\n", kv.first.c_str());
        } else if (t[0] == "buf" && t.size() >= 4) {
            if (g_bufs.count(t[1])) free(g_bufs[t[1]].p);
            Buf b{nullptr, 0};
            if (t[2] == "file") {
                FILE *f = fopen(t[3].c_str(), "rb");
                if (!f) fail("cannot open " + t[3]);
                fseek(f, 0, SEEK_END);
                b.n = (size_t)ftell(f);
                fseek(f, 0, SEEK_SET);
                b.p = exact_block(b.n);
                if (b.n && fread(b.p, 1, b.n, f) != b.n) fail("short read of " + t[3]);
                fclose(f);
            } else if (t[2] == "zero" || (t[2] == "fill" && t.size() == 5)) {
                b.n = (size_t)strtoull(t[3].c_str(), nullptr, 0);
                b.p = exact_block(b.n);
                memset(b.p, t[2] == "fill" ? (int)strtol(t[4].c_str(), nullptr, 0) : 0, b.n);
            } else {
                fail("bad buf command");
            }
            g_bufs[t[1]] = b;
        } else if (t[0] == "call" && t.size() >= 2) {
            const auto it = g_table.find(t[1]);
            if (it == g_table.end()) fail("no entry point named " + t[1]);
            it->second(std::vector<std::string>(t.begin() + 2, t.end()));
        } else if (t[0] == "dump" && t.size() == 3) {
            const auto it = g_bufs.find(t[1]);
            if (it == g_bufs.end()) fail("no buffer named " + t[1]);
            FILE *f = fopen(t[2].c_str(), "wb");
            if (!f) fail("cannot write " + t[2]);
            if (it->second.n && fwrite(it->second.p, 1, it->second.n, f) != it->second.n) fail("short write");
            fclose(f);
        } else {
            fail(std::string("bad command: ") + lineptr);
        }
    }
    free(lineptr);
    for (auto &kv : g_bufs) free(kv.second.p);
    g_bufs.clear();
    free(hostsim::g_lds_arena);
    hostsim::g_lds_arena = nullptr;
    fflush(stdout);
    return 0;
}

}  // namespace driver

int main() { return driver::run(stdin); }
