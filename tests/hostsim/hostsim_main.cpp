// hostsim_main.cpp -- the shipped device sources, launch policy and device-pointer C ABI of hades252_amd/csrc as ONE host
// program, for the CPU-tier tests tests/test_hostsim_*.py (built by tests/hostsim_lib.py with ASan+UBSan, and with TSan).
//
// The include list is that of hades252_amd/csrc/hades252.hip without the host plumbing (host_pin / host_pool / host_pipe /
// host_callers / host_safe / host_cipher); host_fault.hpp stays because the abi_*.hpp files use its HIP_TRY and fault hook.
// <hip/hip_runtime.h> resolves to the stand-in in this directory (block emulator: see there).  The unit kernels of
// tests/units/arith_units.hip come along unchanged.  Nothing in this file does arithmetic or defines a kernel: it is a
// table of entry points, a handful of launchers that reach a shipped kernel form at a size the dispatch would not give it
// (namespace forms), and a script reader.
//
// Script (stdin), one command per line:
//   buf NAME file PATH        NAME = the bytes of PATH, in a heap block of EXACTLY that size (ASan sees byte n)
//   buf NAME zero BYTES       ... or BYTES zero bytes
//   buf NAME fill BYTES V     ... or BYTES bytes of value V
//   call FUNC ARG...          one argument per parameter: a pointer is NAME, NAME+OFFSET or null; an integer is parsed
//                             prints "rc FUNC VALUE"
//                             and, with HOSTSIM_SKIP_NOT_EMULATED=1, "not_emulated FUNC BUILTIN" when a launch met a
//                             builtin the stand-in header has no emulation for (none at present)
//                             and, with HOSTSIM_DPP_MAX_BLOCKS=k, "over_budget FUNC" when a launch of more than k blocks
//                             met a DPP / permlane move and was given up (hip/hip_runtime.h says why)
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

// ---- form launchers -----------------------------------------------------------------------------------------------------
// The size dispatch gives the unhelped one-per-wave form to 769 .. 1 024 states and the per-row form to 1 025 .. 4 096: at
// seconds per emulated block no test can afford those sizes.  Each launcher below launches ONE shipped kernel form with the
// geometry and the arguments of its call site in abi_*.hpp / launch.hpp (copied, and small enough to read side by side), at
// whatever n the script gives.  form: 0 = one per wave with a helper wave, 1 = one per wave without, 2 = one per row.
namespace forms {
enum { kHelped = 0, kUnhelped = 1, kRows = 2 };
static dim3 lanes_grid(size_t n, int form) {
    const unsigned per = form == kHelped ? kLanesWaves - 1 : kLanesWaves;
    return dim3((unsigned)((n + per - 1) / per));
}
static dim3 rows_grid(size_t n) { return dim3((unsigned)((n + kRowsWaves * kRowsPerWave - 1) / (kRowsWaves * kRowsPerWave))); }
static const dim3 kLanesBlock(kLanesWaves *kWave), kRowsBlock(kRowsWaves *kWave);
#define FORM_LAUNCH(form, helped_k, unhelped_k, rows_k, n, ...)                                                  \
    do {                                                                                                         \
        if ((form) == kHelped)                                                                                   \
            hipLaunchKernelGGL(helped_k, lanes_grid((n), kHelped), kLanesBlock, 0, (hipStream_t) nullptr, __VA_ARGS__);   \
        else if ((form) == kUnhelped)                                                                            \
            hipLaunchKernelGGL(unhelped_k, lanes_grid((n), kUnhelped), kLanesBlock, 0, (hipStream_t) nullptr, __VA_ARGS__); \
        else if ((form) == kRows)                                                                                \
            hipLaunchKernelGGL(rows_k, rows_grid(n), kRowsBlock, 0, (hipStream_t) nullptr, __VA_ARGS__);         \
        else                                                                                                     \
            return HADES252_ERR_INVALID_ARG;                                                                     \
    } while (0)

#if HOSTSIM_PART & 1
// abi_perm.hpp: hades252_perm_batch_dev_ex
static int form_perm(uint8_t *states, size_t n, int form) {
    FORM_LAUNCH(form, k_perm_lanes<true>, k_perm_lanes<false>, k_perm_rows, n, states, n);
    return HADES252_OK;
}
#endif
#if HOSTSIM_PART & 2
// launch.hpp: launch_merkle_lanes / launch_merkle_rows
static int form_merkle_level(int arity, const uint8_t *children, size_t n_children, uint8_t *parents, size_t n,
                             const uint64_t *tag_mont, int out_idx, const uint8_t *pad, int form) {
    const Fr tag = fr_from_u64(tag_mont);
#define FORM_LEVEL(A)                                                                                            \
    FORM_LAUNCH(form, (k_merkle_lanes<A, true>), (k_merkle_lanes<A, false>), k_merkle_rows<A>, n, children, n_children, \
                parents, n, tag, out_idx, pad)
    switch (arity) {
        case 1: FORM_LEVEL(1); break;
        case 2: FORM_LEVEL(2); break;
        case 3: FORM_LEVEL(3); break;
        case 4: FORM_LEVEL(4); break;
        default: return HADES252_ERR_INVALID_ARG;
    }
#undef FORM_LEVEL
    return HADES252_OK;
}
// launch.hpp: launch_merkle_update
static int form_merkle_update(int arity, const uint8_t *children, size_t n_children, uint8_t *parents, const uint64_t *indices,
                              size_t n_updates, size_t n_leaves, uint64_t span, const uint64_t *tag_mont, int out_idx,
                              const uint8_t *pad, int form) {
    const Fr tag = fr_from_u64(tag_mont);
#define FORM_UPDATE(A)                                                                                           \
    FORM_LAUNCH(form, (k_merkle_update_lanes<A, true>), (k_merkle_update_lanes<A, false>), k_merkle_update_rows<A>, \
                n_updates, children, n_children, parents, indices, n_updates, n_leaves, span, tag, out_idx, pad)
    switch (arity) {
        case 2: FORM_UPDATE(2); break;
        case 3: FORM_UPDATE(3); break;
        case 4: FORM_UPDATE(4); break;
        default: return HADES252_ERR_INVALID_ARG;
    }
#undef FORM_UPDATE
    return HADES252_OK;
}
// abi_merkle.hpp: hades252_merkle_verify_dev
static int form_merkle_verify(const uint8_t *leaves, const uint64_t *indices, const uint8_t *paths, size_t n_queries,
                              int depth, int arity, const uint64_t *tag_mont, int out_idx, uint8_t *roots, int form) {
    const Fr tag = fr_from_u64(tag_mont);
#define FORM_VERIFY(A)                                                                                           \
    FORM_LAUNCH(form, (k_merkle_verify_lanes<A, true>), (k_merkle_verify_lanes<A, false>), k_merkle_verify_rows<A>, \
                n_queries, leaves, indices, paths, n_queries, depth, tag, out_idx, roots)
    switch (arity) {
        case 1: FORM_VERIFY(1); break;
        case 2: FORM_VERIFY(2); break;
        case 3: FORM_VERIFY(3); break;
        case 4: FORM_VERIFY(4); break;
        default: return HADES252_ERR_INVALID_ARG;
    }
#undef FORM_VERIFY
    return HADES252_OK;
}
#endif
#if HOSTSIM_PART & 4
// abi_sponge.hpp: sponge_launch
static int form_sponge(const uint8_t *scalars, const uint64_t *offsets, const uint64_t *lengths, size_t n_msgs,
                       size_t fixed_len, const uint64_t *capacity_mont, int pad_mode, uint8_t *digests, size_t n_scalars,
                       int *bad_count, int form) {
    FORM_LAUNCH(form, k_sponge_lanes<true>, k_sponge_lanes<false>, k_sponge_rows, n_msgs, scalars, offsets, lengths, digests,
                n_msgs, fixed_len, fr_from_u64(capacity_mont), pad_mode, n_scalars, bad_count);
    return HADES252_OK;
}
// abi_sponge.hpp: hades252_sponge_absorb_dev
static int form_sponge_absorb(uint8_t *states, const uint8_t *blocks, size_t n, int blocks_each, int form) {
    FORM_LAUNCH(form, k_sponge_absorb_lanes<true>, k_sponge_absorb_lanes<false>, k_sponge_absorb_rows, n, states, blocks, n,
                blocks_each);
    return HADES252_OK;
}
// abi_cipher.hpp: cipher_launch (there is no per-row cipher)
static int form_cipher(int decrypt, const uint8_t *in, const uint8_t *keys, const uint8_t *nonces, size_t n, size_t len,
                       const uint64_t *domain_mont, uint8_t *out, uint8_t *ok, int *rejected, int form) {
    const Fr dom = fr_from_u64(domain_mont), lw = fr_mont_of_u64(len);
    if (form == kRows) return HADES252_ERR_INVALID_ARG;
    if (decrypt)
        FORM_LAUNCH(form, (k_cipher_lanes<true, true>), (k_cipher_lanes<true, false>), (k_cipher_lanes<true, false>), n, in,
                    keys, nonces, out, ok, rejected, n, len, dom, lw);
    else
        FORM_LAUNCH(form, (k_cipher_lanes<false, true>), (k_cipher_lanes<false, false>), (k_cipher_lanes<false, false>), n, in,
                    keys, nonces, out, ok, rejected, n, len, dom, lw);
    return HADES252_OK;
}
// abi_safe.hpp: safe_launch behind hades252_safe_hash_dev (states == NULL) and safe_stream (one call from *cursor on)
static int form_safe(const uint8_t *in, uint8_t *out, uint8_t *states, size_t n, const uint32_t *calls, size_t n_calls,
                     uint32_t *cursor, const uint64_t *tag_mont, int form) {
    SafePlan plan;
    const uint32_t start = cursor != nullptr ? *cursor : 0;
    if (form == kRows || !safe_plan(calls, n_calls, start, plan)) return HADES252_ERR_INVALID_ARG;
    const Fr tag = tag_mont != nullptr ? fr_from_u64(tag_mont) : Fr{};
    FORM_LAUNCH(form, k_safe_lanes<true>, k_safe_lanes<false>, k_safe_lanes<false>, n, in, out, states, n, plan.n_in, plan.n_out,
                plan.calls, plan.n_calls, start, plan.n_perms, tag);
    if (cursor != nullptr) *cursor = plan.cursor_out;
    return HADES252_OK;
}
#endif
#undef FORM_LAUNCH
}  // namespace forms
using namespace forms;
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
        if (hostsim::g_over_budget.exchange(false)) printf("over_budget %s\n", name);
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
    // ... and the forms whose dispatch sizes cost minutes here (above)
    REG(form_perm);
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
    REG(form_merkle_level); REG(form_merkle_update); REG(form_merkle_verify);
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
    REG(form_sponge); REG(form_sponge_absorb); REG(form_cipher); REG(form_safe);
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
    // tests/units/arith_units.hip
    REG(units_to_f29); REG(units_from_f29); REG(units_mont_mul); REG(units_mont_sqr); REG(units_mont_mul_const);
    REG(units_mont_mul_small); REG(units_mont_lin); REG(units_mont_lin1); REG(units_sbox29); REG(units_add_lazy);
    REG(units_small_mds); REG(units_finalize); REG(units_finalize1); REG(units_finalize32); REG(units_mds_row_cols);
    REG(units_fr_add); REG(units_fr_cond_sub_p); REG(units_fr_mul); REG(units_fr_is_canonical);
    REG(units_lane_mont_mul); REG(units_lane_sbox); REG(units_lane_lin); REG(units_lane_mds_row); REG(units_carry_split);
    REG(units_dpp_moves);
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
