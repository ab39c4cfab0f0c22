// host_grind.hpp -- C ABI, HOST memory in and out: batched proof-of-work grinding (kernels_grind.hpp).  A job is 160 bytes
// in and 9 bytes out, so there is no device-pointer form: the seeds are uploaded once, the search runs in rounds of one
// launch each and 8 bytes per job come back after every round.
#pragma once

extern "C" {

// Candidates per launch, all jobs together: each job gets an equal share of it as its window of the round (a multiple of
// 256, at least 256).  Larger windows pay fewer launches and slot downloads per candidate; smaller ones leave less work in
// flight when a hit lands (the in-kernel early exit stops waves that have not started their range, not the ones that have).
// Chosen by measurement (profiles/f10_grind/README.md): 2^24 has the smallest median overhead over the ideal time to
// solution of the four windows tried (2^20 .. 2^26) and the full throughput (1.02 x k_perm_fast in the same run).
static constexpr uint64_t kGrindWindow = (uint64_t)1 << 24;
// Iterations of a lane: one block covers kGrindIters * 256 consecutive nonces of its job's window.  The blocks resident at
// one time work on nonces spread over kGrindIters times their number, so a hit waits for iterations of larger nonces.
// Measured with 1, 4 and 16: the throughput is the same (1.02 x k_perm_fast), a hit near 2^20 comes back after 0.7 / 1.0 /
// 2.5 ms over the ideal: one iteration, as k_perm_fast runs one state per lane (profiles/f10_grind/README.md).
static constexpr uint32_t kGrindIters = 1;
// Test hook: HADES252_TEST_GRIND_WINDOW (read once, at the first call) lowers the window so that the loop's later rounds run
// on a few thousand candidates (tests/test_gpu_f10_grind.py); values below 256 (less than one block per job: a stray
// setting would turn a call into millions of launches) are ignored.
static uint64_t grind_window() {
    static const uint64_t v = []() -> uint64_t {
        const char *e = getenv("HADES252_TEST_GRIND_WINDOW");
        const uint64_t t = e ? (uint64_t)strtoull(e, nullptr, 0) : 0;
        return t >= 256 && t < kGrindWindow ? t : kGrindWindow;
    }();
    return v;
}

int hades252_grind(const uint64_t *seeds, size_t n_jobs, int word, int out_idx, const uint64_t target[4], uint64_t first_nonce,
                   uint64_t max_nonces, uint64_t *nonces, uint8_t *found) {
    if (n_jobs == 0) return HADES252_OK;
    if (seeds == nullptr || target == nullptr || nonces == nullptr || found == nullptr || word < 0 || word > 4 ||
        out_idx < 0 || out_idx > 4 || n_jobs > HADES252_GRIND_MAX_JOBS ||
        (first_nonce != 0 && max_nonces > 0 - first_nonce))               // (the last: first_nonce + max_nonces > 2^64)
        return HADES252_ERR_INVALID_ARG;
    if (max_nonces == 0) {
        memset(found, 0, n_jobs);
        return HADES252_OK;
    }
    int rc = check_device();
    if (rc != HADES252_OK) return rc;
    GrindTarget tgt;
    for (int k = 0; k < 4; k++) {
        tgt.l[2 * k] = (uint32_t)target[k];
        tgt.l[2 * k + 1] = (uint32_t)(target[k] >> 32);
    }
    // one job's window per round: its share of the launch, a whole number of blocks' first iterations
    uint64_t per_job = grind_window() / n_jobs;
    per_job = per_job < kBlock ? kBlock : (per_job + kBlock - 1) / kBlock * kBlock;
    const size_t seeds_b = n_jobs * 160, slots_b = n_jobs * 8;
    std::vector<uint64_t> h_slots(n_jobs, UINT64_MAX);                     // all-ones: no hit yet
    HostCall call;
    rc = call.acquire(16);
    if (rc != HADES252_OK) return rc;
    HostPipe &pp = call.pipe;
    rc = pipe_ensure_aux(pp, seeds_b + slots_b + 16);
    if (rc != HADES252_OK) return call.finish(rc);
    uint8_t *d_seeds = (uint8_t *)pp.aux, *d_slots = d_seeds + seeds_b;
    const hipStream_t s = pp.s_k;
    TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_seeds, seeds, seeds_b, hipMemcpyHostToDevice, s)));
    TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(d_slots, h_slots.data(), slots_b, hipMemcpyHostToDevice, s)));
    for (uint64_t off = 0; off < max_nonces;) {
        const uint64_t count = max_nonces - off < per_job ? max_nonces - off : per_job;
        const uint64_t trips = (count + kBlock - 1) / kBlock;             // iterations the window holds, over all its blocks
        const uint32_t iters = trips < kGrindIters ? (uint32_t)trips : kGrindIters;
        const dim3 grid((unsigned)((trips + iters - 1) / iters), (unsigned)n_jobs);
        hipLaunchKernelGGL(k_grind, grid, dim3(kBlock), 0, s, (const uint32_t *)d_seeds, (unsigned long long *)d_slots, tgt,
                           word, out_idx, first_nonce, off, count, iters);
        TRY_CALL(call, hipGetLastError());
        TRY_CALL(call, F(F_MEMCPY, hipMemcpyAsync(h_slots.data(), d_slots, slots_b, hipMemcpyDeviceToHost, s)));
        TRY_CALL(call, F(F_SYNC, hipStreamSynchronize(s)));
        off += count;
        bool all_found = true;
        for (size_t j = 0; j < n_jobs && all_found; j++) all_found = h_slots[j] != UINT64_MAX;
        if (all_found) break;
    }
    for (size_t j = 0; j < n_jobs; j++) {
        found[j] = h_slots[j] != UINT64_MAX;
        if (found[j]) nonces[j] = first_nonce + h_slots[j];
    }
    return call.finish(HADES252_OK);
}

}  // extern "C"
