// hip/hip_runtime.h -- host stand-in for the HIP runtime header (tests/hostsim_lib.py puts this directory first on the
// include path).  Test infrastructure only: it lets the SHIPPED device sources and launch policy of hades252_amd/csrc
// compile for the CPU and run under the host sanitizers.  Nothing here does field arithmetic or defines a kernel.
//
// Block emulator: the blocks of a launch run one after another; the threads of a block are real OS threads.
//   __syncthreads()                    barrier over the block's live threads
//   __builtin_amdgcn_wave_barrier()    barrier over the live threads of a 64-thread wave
//   __ballot / __shfl* / readlane / readfirstlane   one exchange slot per wave, between two wave barriers
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
    uint64_t slot[kWaveSize];            // the exchange slot of ballot / shuffle / readlane
};

struct Block {
    Barrier bar;
    std::vector<Wave> waves;
    explicit Block(unsigned n_threads) : waves((n_threads + kWaveSize - 1) / kWaveSize) {
        bar.set_live(n_threads);
        for (unsigned w = 0; w < waves.size(); w++) {
            const unsigned n = n_threads - w * kWaveSize < kWaveSize ? n_threads - w * kWaveSize : kWaveSize;
            waves[w].bar.set_live(n);
            waves[w].alive.store(n == kWaveSize ? ~0ull : (1ull << n) - 1);
        }
    }
};

struct Ctx {
    Block *block = nullptr;
    Wave *wave = nullptr;
    int lane = 0;
};
inline thread_local Ctx tl_ctx;
inline uint8_t *g_lds_arena = nullptr;

[[noreturn]] inline void die(const char *what, const char *name) {
    fprintf(stderr, "hostsim: %s: %s\n", what, name);
    fflush(stderr);
    abort();
}
// The one-state-per-wave and per-row forms (hades_lanes.hpp) move data with DPP / permlane and read s_memtime; they are
// not emulated.  Their builtins are declared so that the unit compiles, and reaching one ends the run.
struct Pair {
    uint32_t v[2];
    uint32_t operator[](int i) const { return v[i]; }
};
// With HOSTSIM_SKIP_NOT_EMULATED=1 in the environment the launch is given up instead (its outputs stay as they were), the
// driver reports it and the run goes on: a whole tree's large levels can then be checked although its small levels run a
// DPP form.
struct NotEmulated {
    const char *name;
};
inline std::atomic<const char *> g_not_emulated{nullptr};
[[noreturn]] inline void not_emulated(const char *name) {
    static const bool skip = getenv("HOSTSIM_SKIP_NOT_EMULATED") != nullptr;
    if (!skip) die("form not emulated (needs DPP/permlane/s_memtime)", name);
    throw NotEmulated{name};
}
[[noreturn]] inline int not_emulated_int(const char *name) { not_emulated(name); }
[[noreturn]] inline Pair not_emulated_pair(const char *name) { not_emulated(name); }
[[noreturn]] inline unsigned long long not_emulated_u64(const char *name) { not_emulated(name); }

inline uint8_t *dynamic_lds() { return g_lds_arena; }
inline void syncthreads() { tl_ctx.block->bar.arrive_and_wait(); }
inline void wave_barrier() { tl_ctx.wave->bar.arrive_and_wait(); }

// publish my value, wait for the wave, let `read` look at the slots, wait again before anyone overwrites them
template <class F>
inline uint64_t exchange(uint64_t mine, F read) {
    Wave &w = *tl_ctx.wave;
    w.slot[tl_ctx.lane] = mine;
    w.bar.arrive_and_wait();
    const uint64_t r = read(w.slot, w.alive.load());
    w.bar.arrive_and_wait();
    return r;
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
    return from_bits<T>(exchange(to_bits(v), [from](const uint64_t *s, uint64_t alive) {
        return (alive >> from) & 1 ? s[from] : 0;
    }));
}
template <class T>
inline T shfl_down(T v, unsigned delta, int width) {
    const int lane = tl_ctx.lane;
    const int from = lane + (int)delta;
    const bool own = (from & ~(width - 1)) != (lane & ~(width - 1));      // past the group's end: keeps its own value
    const uint64_t mine = to_bits(v);
    return from_bits<T>(exchange(mine, [=](const uint64_t *s, uint64_t alive) {
        return own ? mine : ((alive >> from) & 1 ? s[from] : 0);
    }));
}
inline uint64_t ballot(int pred) {
    return exchange(pred ? 1 : 0, [](const uint64_t *s, uint64_t alive) {
        uint64_t m = 0;
        for (int i = 0; i < kWaveSize; i++)
            if (((alive >> i) & 1) && s[i]) m |= 1ull << i;
        return m;
    });
}
template <class T>
inline T readfirstlane(T v) {
    return from_bits<T>(exchange(to_bits(v), [](const uint64_t *s, uint64_t alive) { return s[__builtin_ctzll(alive)]; }));
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
                try {
                    run();
                } catch (const NotEmulated &e) {
                    g_not_emulated.store(e.name);
                }
                // returned (early or at the end): no barrier waits for this lane any more, no exchange sees it
                tl_ctx.wave->alive.fetch_and(~(1ull << tl_ctx.lane));
                tl_ctx.wave->bar.leave();
                blk.bar.leave();
            });
        for (auto &th : threads) th.join();
        if (g_not_emulated.load() != nullptr) break;                     // a launch that met a DPP form is given up
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
#define __builtin_amdgcn_update_dpp(...) hostsim::not_emulated_int("__builtin_amdgcn_update_dpp")
#define __builtin_amdgcn_permlane16_swap(...) hostsim::not_emulated_pair("__builtin_amdgcn_permlane16_swap")
#define __builtin_amdgcn_permlane32_swap(...) hostsim::not_emulated_pair("__builtin_amdgcn_permlane32_swap")
#define __builtin_amdgcn_s_memtime() hostsim::not_emulated_u64("__builtin_amdgcn_s_memtime")

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
