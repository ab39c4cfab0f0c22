// hip/hip_runtime.h -- host stand-in for the HIP runtime header (tests/hostsim_lib.py puts this directory first on the
// include path).  Test infrastructure only: it lets the SHIPPED device sources and launch policy of hades252_amd/csrc
// compile for the CPU and run under the host sanitizers.  Nothing here does field arithmetic or defines a kernel.
//
// Block emulator: the blocks of a launch run one after another; the threads of a block are real OS threads.
//   __syncthreads()                    barrier over the block's live threads
//   __builtin_amdgcn_wave_barrier()    barrier over the live threads of a 64-thread wave
//   __ballot / __shfl* / readlane / readfirstlane   an exchange through the wave's slots and one wave barrier
//   update_dpp (row_shl / row_shr / row_newbcast), permlane16_swap / permlane32_swap   the same: one exchange per move
//   atomicAdd                          __atomic builtins
// A thread that returns from the kernel leaves every barrier's participant count and counts as an inactive lane.
// `__shared__` objects are function-level statics: one per block, because blocks run one at a time.  The dynamic LDS of a
// launch is a window of the requested size at the front of an arena whose rest is poisoned for AddressSanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits.h>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <atomic>
#include <thread>
#include <vector>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define HOSTSIM_ASAN 1
#endif
#endif
#ifndef HOSTSIM_ASAN
#define ASAN_POISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#endif

// ---- qualifiers ---------------------------------------------------------------------------------------------------
#define __host__
#define __device__
#define __global__ static
#define __constant__
#define __shared__ static
#define __forceinline__ inline __attribute__((always_inline))
#define __noinline__ __attribute__((noinline))
#define __launch_bounds__(...)

// ---- vector types, launch geometry ----------------------------------------------------------------------------------
struct alignas(16) uint4 {
    unsigned x, y, z, w;
};
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }
struct uint3 {
    unsigned x, y, z;
};
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

namespace hostsim {

constexpr int kWaveSize = 64;
// dynamic LDS arena: the 160 KiB a gfx950 workgroup can address; a launch sees only the window it asked for
constexpr size_t kLdsArena = 160 * 1024;

// A barrier over however many participants are still alive (a pthread_barrier would wait for ever for a lane that has
// returned from the kernel).  The count of live participants and of those waiting share one atomic word; waiters sleep
// on the generation word through the futex call and take no lock when they wake: with a mutex every one of the 319
// sleepers of a 320-thread block queues for it again on wake-up.  The sanitizers see the ordering through the acquire /
// release operations on the two atomics.
struct Barrier {
    std::atomic<uint64_t> state{0};      // live << 32 | waiting
    std::atomic<uint32_t> gen{0};
    void set_live(unsigned n) { state.store((uint64_t)n << 32); }
    void release() {
        gen.fetch_add(1, std::memory_order_acq_rel);
        syscall(SYS_futex, (uint32_t *)&gen, FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
    }
    void arrive_and_wait() {
        const uint32_t g = gen.load(std::memory_order_acquire);
        uint64_t s = state.load(std::memory_order_acquire);
        for (;;) {
            const uint32_t live = (uint32_t)(s >> 32), waiting = (uint32_t)s;
            if (waiting + 1 == live) {                                   // the last one in: nobody waits any more
                if (state.compare_exchange_weak(s, (uint64_t)live << 32, std::memory_order_acq_rel)) {
                    release();
                    return;
                }
            } else if (state.compare_exchange_weak(s, s + 1, std::memory_order_acq_rel)) {
                break;
            }
        }
        while (gen.load(std::memory_order_acquire) == g)
            syscall(SYS_futex, (uint32_t *)&gen, FUTEX_WAIT_PRIVATE, g, nullptr, nullptr, 0);
    }
    void leave() {
        uint64_t s = state.load(std::memory_order_acquire);
        for (;;) {
            const uint32_t live = (uint32_t)(s >> 32) - 1, waiting = (uint32_t)s;
            const bool done = live > 0 && waiting == live;               // everyone still alive is already waiting
            if (state.compare_exchange_weak(s, done ? (uint64_t)live << 32 : ((uint64_t)live << 32 | waiting),
                                            std::memory_order_acq_rel)) {
                if (done) release();
                return;
            }
        }
    }
};

struct Wave {
    Barrier bar;
    std::atomic<uint64_t> alive{0};      // lanes that have not returned from the kernel
    uint64_t full = 0;                   // the lanes the wave started with
    uint64_t slot[2][kWaveSize] = {};    // the exchange slots of ballot / shuffle / readlane / DPP, used alternately
    uint32_t stamp[2][kWaveSize] = {};   // ... and the number of the exchange each entry was written for
};

struct Block {
    Barrier bar;
    std::vector<Wave> waves;
    explicit Block(unsigned n_threads) : waves((n_threads + kWaveSize - 1) / kWaveSize) {
        bar.set_live(n_threads);
        for (unsigned w = 0; w < waves.size(); w++) {
            const unsigned n = n_threads - w * kWaveSize < kWaveSize ? n_threads - w * kWaveSize : kWaveSize;
            waves[w].bar.set_live(n);
            waves[w].full = n == kWaveSize ? ~0ull : (1ull << n) - 1;
            waves[w].alive.store(waves[w].full);
        }
    }
};

struct Ctx {
    Block *block = nullptr;
    Wave *wave = nullptr;
    int lane = 0;
    unsigned grid_blocks = 0;
    unsigned exchanges = 0;              // how many exchanges this lane has taken part in: picks the slot buffer
};
inline thread_local Ctx tl_ctx;
inline uint8_t *g_lds_arena = nullptr;

[[noreturn]] inline void die(const char *what, const char *name) {
    fprintf(stderr, "hostsim: %s: %s\n", what, name);
    fflush(stderr);
    abort();
}
// what the permlane swaps return: element 0 is the new first operand, element 1 the new second
struct Pair {
    uint32_t v[2];
    uint32_t operator[](int i) const { return v[i]; }
};
// For a builtin that has no emulation (none at present: tests/hostsim/not_emulated.json is empty): it is declared through
// one of these so that the unit compiles, and reaching it ends the run.  With HOSTSIM_SKIP_NOT_EMULATED=1 in the
// environment the launch is given up instead (its outputs stay as they were), the driver reports it and the run goes on.
struct NotEmulated {
    const char *name;
};
inline std::atomic<const char *> g_not_emulated{nullptr};
[[noreturn]] inline void not_emulated(const char *name) {
    static const bool skip = getenv("HOSTSIM_SKIP_NOT_EMULATED") != nullptr;
    if (!skip) die("form not emulated", name);
    throw NotEmulated{name};
}
[[noreturn]] inline int not_emulated_int(const char *name) { not_emulated(name); }
[[noreturn]] inline Pair not_emulated_pair(const char *name) { not_emulated(name); }
[[noreturn]] inline unsigned long long not_emulated_u64(const char *name) { not_emulated(name); }

inline uint8_t *dynamic_lds() { return g_lds_arena; }
inline void syncthreads() { tl_ctx.block->bar.arrive_and_wait(); }
inline void wave_barrier() { tl_ctx.wave->bar.arrive_and_wait(); }

// Publish my value, wait for the wave, let `read` look at the slots.  ONE barrier per exchange: consecutive exchanges use
// the two slot buffers alternately, so the buffer of exchange i is written again in exchange i + 2 at the earliest, and a
// lane gets there only through the barrier of exchange i + 1, at which every lane arrives after its reads of exchange i.
// (Every live lane of a wave takes part in every exchange -- the barrier would not open otherwise -- so the lanes' counts
// agree.)  A lane is active in an exchange if its entry carries the exchange's number: a lane that has returned from the
// kernel left an older one, and a lane that returns right after its own reads still counts for the slower readers.
// A permutation of hades_lanes.hpp is ~13 000 exchanges: a second barrier behind the reads was half of its cost here.
struct Slots {
    const uint64_t *value;
    const uint32_t *stamp;
    uint32_t number;
    bool active(int lane) const { return stamp[lane] == number; }
    uint64_t active_mask() const {
        uint64_t m = 0;
        for (int i = 0; i < kWaveSize; i++) m |= (uint64_t)active(i) << i;
        return m;
    }
};
template <class F>
inline uint64_t exchange(uint64_t mine, F read) {
    Wave &w = *tl_ctx.wave;
    const uint32_t number = ++tl_ctx.exchanges;
    const int buf = number & 1;
    w.slot[buf][tl_ctx.lane] = mine;
    w.stamp[buf][tl_ctx.lane] = number;
    w.bar.arrive_and_wait();
    return read(Slots{w.slot[buf], w.stamp[buf], number});
}
template <class T>
inline uint64_t to_bits(T v) {
    static_assert(sizeof(T) <= 8, "exchange slot holds 64 bits");
    uint64_t b = 0;
    memcpy(&b, &v, sizeof(T));
    return b;
}
template <class T>
inline T from_bits(uint64_t b) {
    T v;
    memcpy(&v, &b, sizeof(T));
    return v;
}
// value of lane `src` of my `width`-lane group; an inactive source lane reads as zero (what ds_bpermute returns)
template <class T>
inline T shfl(T v, int src, int width) {
    const int lane = tl_ctx.lane;
    const int from = (lane & ~(width - 1)) | (src & (width - 1));
    return from_bits<T>(exchange(to_bits(v), [from](const Slots &s) { return s.active(from) ? s.value[from] : 0; }));
}
template <class T>
inline T shfl_down(T v, unsigned delta, int width) {
    const int lane = tl_ctx.lane;
    const int from = lane + (int)delta;
    const bool own = (from & ~(width - 1)) != (lane & ~(width - 1));      // past the group's end: keeps its own value
    const uint64_t mine = to_bits(v);
    return from_bits<T>(exchange(mine, [=](const Slots &s) { return own ? mine : (s.active(from) ? s.value[from] : 0); }));
}
inline uint64_t ballot(int pred) {
    return exchange(pred ? 1 : 0, [](const Slots &s) {
        uint64_t m = 0;
        for (int i = 0; i < kWaveSize; i++)
            if (s.active(i) && s.value[i]) m |= 1ull << i;
        return m;
    });
}
template <class T>
inline T readfirstlane(T v) {
    return from_bits<T>(exchange(to_bits(v), [](const Slots &s) { return s.value[__builtin_ctzll(s.active_mask())]; }));
}

// ---- DPP and permlane moves (hades_lanes.hpp): each is ONE wave-wide exchange, the lockstep of a wave as __shfl has it.
// The hardware's rules for a source lane that is switched off differ per instruction (and per bound_ctrl / fi); no shipped
// form runs one of these with a lane it could read from gone, so a move that could read a lane that has returned from the
// kernel ends the run instead of guessing.  `lanes`: what the move of this lane's group can read -- the whole wave for the
// permlane swaps, the lane's own 16-lane row for the DPP row moves (a row move never leaves its row, so which lanes of
// OTHER rows are on cannot matter: the unit wrappers of tests/units/arith_units.hip retire whole rows past n).
// Every one of these moves is a wave barrier of 64 OS threads, and a permutation of hades_lanes.hpp is ~13 000 of them: a
// block takes seconds.  A whole tree's small levels (up to 4 096 parents: a thousand such blocks) are out of any test's
// reach, so with HOSTSIM_DPP_MAX_BLOCKS=k in the environment a launch of MORE than k blocks that executes such a move is
// given up (its outputs stay as they were), the driver reports "over_budget" and the run goes on: the large levels of a
// tree can then be checked on their own.  Unset: no limit.
struct OverBudget {};
inline std::atomic<bool> g_over_budget{false};
inline void dpp_budget() {
    static const long limit = [] {
        const char *e = getenv("HOSTSIM_DPP_MAX_BLOCKS");
        return e != nullptr ? strtol(e, nullptr, 0) : -1L;
    }();
    if (limit >= 0 && (long)tl_ctx.grid_blocks > limit) throw OverBudget{};
}
inline void need_lanes(const Slots &s, uint64_t lanes, const char *name) {
    lanes &= tl_ctx.wave->full;
    if ((s.active_mask() & lanes) != lanes) die("a lane the move reads had returned from the kernel when the wave executed", name);
}
// v_mov_b32_dpp with row_mask = bank_mask = 0xF and bound_ctrl: the row moves of a 16-lane row, zero from outside the row
inline int update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
    static const char *const name = "__builtin_amdgcn_update_dpp";
    dpp_budget();
    (void)old;                                                           // with bound_ctrl no lane keeps its old value
    if (row_mask != 0xF || bank_mask != 0xF || !bound_ctrl) die("masks other than 0xF/0xF, or bound_ctrl off, are not emulated", name);
    const int lane = tl_ctx.lane, k = lane & 15, row0 = lane & ~15;
    int from;
    if (ctrl >= 0x101 && ctrl <= 0x10F) from = k + (ctrl - 0x100);       // row_shl:n   lane k <- lane k + n
    else if (ctrl >= 0x111 && ctrl <= 0x11F) from = k - (ctrl - 0x110);  // row_shr:n   lane k <- lane k - n
    else if (ctrl >= 0x150 && ctrl <= 0x15F) from = ctrl - 0x150;        // row_newbcast:n
    else die("DPP control not emulated (only the row shifts and the row broadcast)", name);
    const bool in_row = from >= 0 && from < 16;
    return (int)(uint32_t)exchange((uint32_t)src, [=](const Slots &s) -> uint64_t {
        need_lanes(s, 0xFFFFull << row0, name);
        return in_row ? s.value[row0 + from] : 0;
    });
}
// v_permlane16_swap d, s: rows 1, 3 of d <-> rows 0, 2 of s (HALF = 16); v_permlane32_swap: rows 2, 3 of d <-> rows 0, 1
// of s (HALF = 32).  Both operands travel in one slot (d low, s high); the result is {new d, new s}.
template <int HALF>
inline Pair permlane_swap(uint32_t d, uint32_t s, bool fi, bool bound_ctrl, const char *name) {
    if (fi || bound_ctrl) die("fi / bound_ctrl are not emulated", name);
    dpp_budget();
    const int lane = tl_ctx.lane;
    const bool upper = (lane & HALF) != 0;                               // an upper half of d's, a lower half of s's
    const uint64_t r = exchange((uint64_t)d | (uint64_t)s << 32, [=](const Slots &sl) -> uint64_t {
        need_lanes(sl, ~0ull, name);
        const uint64_t mine = sl.value[lane], peer = sl.value[lane ^ HALF];
        // upper half: d <- the peer's s, s stays;  lower half: s <- the peer's d, d stays
        return upper ? (peer >> 32) | (mine & 0xFFFFFFFF00000000ull) : (mine & 0xFFFFFFFFull) | (peer << 32);
    });
    return Pair{{(uint32_t)r, (uint32_t)(r >> 32)}};
}
// s_memtime: only reached with stamps != nullptr (diagnostic builds); a process-wide counter
inline unsigned long long memtime() {
    static std::atomic<unsigned long long> ticks{0};
    return ticks.fetch_add(1, std::memory_order_relaxed);
}

// `run` is the kernel call of one thread (hipLaunchKernelGGL below binds the arguments)
template <class F>
inline void launch(dim3 grid, dim3 block, size_t lds_bytes, F run);

}  // namespace hostsim

inline thread_local uint3 threadIdx, blockIdx;
inline thread_local dim3 blockDim, gridDim;

namespace hostsim {
template <class F>
inline void launch(dim3 grid, dim3 block, size_t lds_bytes, F run) {
    if (lds_bytes > kLdsArena) die("launch asks for more dynamic LDS than a workgroup has", "hipLaunchKernelGGL");
    if (grid.y != 1 || grid.z != 1 || block.y != 1 || block.z != 1) die("only 1-D launches are emulated", "hipLaunchKernelGGL");
    if (g_lds_arena == nullptr && posix_memalign((void **)&g_lds_arena, 16, kLdsArena) != 0) die("out of memory", "lds");
    ASAN_UNPOISON_MEMORY_REGION(g_lds_arena, kLdsArena);
    ASAN_POISON_MEMORY_REGION(g_lds_arena + lds_bytes, kLdsArena - lds_bytes);
    for (unsigned b = 0; b < grid.x; b++) {
        Block blk(block.x);
        std::vector<std::thread> threads;
        threads.reserve(block.x);
        for (unsigned t = 0; t < block.x; t++)
            threads.emplace_back([&, t, b] {
                threadIdx = uint3{t, 0, 0};
                blockIdx = uint3{b, 0, 0};
                blockDim = block;
                gridDim = grid;
                tl_ctx.block = &blk;
                tl_ctx.wave = &blk.waves[t / kWaveSize];
                tl_ctx.lane = (int)(t % kWaveSize);
                tl_ctx.grid_blocks = grid.x;
                tl_ctx.exchanges = 0;
                try {
                    run();
                } catch (const NotEmulated &e) {
                    g_not_emulated.store(e.name);
                } catch (const OverBudget &) {
                    g_over_budget.store(true);
                }
                // returned (early or at the end): no barrier waits for this lane any more, no exchange sees it
                tl_ctx.wave->alive.fetch_and(~(1ull << tl_ctx.lane));
                tl_ctx.wave->bar.leave();
                blk.bar.leave();
            });
        for (auto &th : threads) th.join();
        if (g_not_emulated.load() != nullptr || g_over_budget.load()) break;    // the launch is given up
    }
    ASAN_UNPOISON_MEMORY_REGION(g_lds_arena, kLdsArena);
}
}  // namespace hostsim

// ---- device intrinsics ------------------------------------------------------------------------------------------------
#define __syncthreads() hostsim::syncthreads()
#define __builtin_amdgcn_wave_barrier() hostsim::wave_barrier()
// the scope string names a hardware scope; on the host every fence is a full thread fence of the given order
#define __builtin_amdgcn_fence(order, scope) std::atomic_thread_fence((std::memory_order)(order))
// scheduling hint to the gfx950 instruction scheduler: no run-time meaning
#define __builtin_amdgcn_sched_barrier(mask) ((void)(mask))
#define __builtin_amdgcn_readfirstlane(v) hostsim::readfirstlane(v)
#define __builtin_amdgcn_readlane(v, lane) hostsim::shfl((v), (lane), hostsim::kWaveSize)
#define __builtin_amdgcn_alignbit(hi, lo, sh) ((uint32_t)((((uint64_t)(hi) << 32) | (uint32_t)(lo)) >> ((sh) & 31)))
#define __builtin_amdgcn_update_dpp(old, src, ctrl, row_mask, bank_mask, bound_ctrl) \
    hostsim::update_dpp((old), (src), (ctrl), (row_mask), (bank_mask), (bound_ctrl))
#define __builtin_amdgcn_permlane16_swap(d, s, fi, bc) hostsim::permlane_swap<16>((d), (s), (fi), (bc), "__builtin_amdgcn_permlane16_swap")
#define __builtin_amdgcn_permlane32_swap(d, s, fi, bc) hostsim::permlane_swap<32>((d), (s), (fi), (bc), "__builtin_amdgcn_permlane32_swap")
#define __builtin_amdgcn_s_memtime() hostsim::memtime()

template <class T>
static inline T __shfl(T v, int src, int width = hostsim::kWaveSize) { return hostsim::shfl(v, src, width); }
template <class T>
static inline T __shfl_down(T v, unsigned delta, int width = hostsim::kWaveSize) { return hostsim::shfl_down(v, delta, width); }
static inline uint64_t __ballot(int pred) { return hostsim::ballot(pred); }
static inline int __any(int pred) { return hostsim::ballot(pred) != 0; }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
template <class T, class U>
static inline T atomicAdd(T *p, U v) { return __atomic_fetch_add(p, (T)v, __ATOMIC_RELAXED); }

// ---- the runtime calls of launch.hpp and abi_*.hpp: host memory stands in for device memory ----------------------------
typedef void *hipStream_t;
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
enum { hipStreamNonBlocking = 1 };
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
static inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) {
    memcpy(d, s, n);
    return hipSuccess;
}
static inline hipError_t hipMalloc(void **p, size_t n) { return posix_memalign(p, 16, n) == 0 ? hipSuccess : hipErrorOutOfMemory; }
static inline hipError_t hipFree(void *p) { free(p); return hipSuccess; }
static inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = nullptr; return hipSuccess; }
static inline hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
// arguments are bound by value, as a launch copies them
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, ...) \
    hostsim::launch(dim3(grid), dim3(block), (size_t)(lds_bytes), [=]() { kernel(__VA_ARGS__); })
