/*
 * hades252.h -- C ABI of libhades252 (MI355X / gfx950 batched Hades252 permutation).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference (dusk-hades 0.24.1)
 * has no FFI of its own; every entry point below names the reference interface it stands in
 * for (paths relative to the reference crate root).  A Rust `Strategy<BlsScalar>` implementor
 * binds these with a plain `extern "C"` block -- see INTEGRATION.md.
 *
 * Data formats
 *   "Montgomery limbs": the in-memory `BlsScalar` -- 4 x u64 little-endian limbs of
 *       value * 2^256 mod p, fully reduced to [0, p).  A state is WIDTH = 5 scalars = 20 u64 =
 *       160 bytes; a batch is an array of states (AoS), permutation i at u64 offset 20*i.
 *       This is exactly `&mut [BlsScalar]` with len = 5*n (zero-copy from Rust).
 *   "canonical bytes": `BlsScalar::to_bytes()` -- 32 little-endian bytes of the value in [0, p)
 *       (the format used at src/round_constants.rs:61-62).
 *   Inputs that are not fully reduced are outside the reference's type invariant; the limb entry
 *   points do not check them, the byte entry points reject them (HADES252_ERR_NOT_CANONICAL).
 *
 * Conventions
 *   - All functions return HADES252_OK (0) or a negative HADES252_ERR_* code; nothing throws or
 *     unwinds across the boundary (the reference builds with panic = 'abort', Cargo.toml:20).
 *   - The caller owns every buffer.  Host-pointer functions are synchronous and keep no
 *     pointer after returning.  `_dev` functions take device pointers valid on the CURRENT HIP
 *     device, enqueue on `stream` (a hipStream_t, NULL = default stream) and return without
 *     synchronising; buffers must stay alive until the stream has drained.  Device pointers must
 *     be 16-byte aligned (hipMalloc'ed buffers and whole-state offsets into them are); host
 *     pointers need only their natural 8-byte alignment.
 *   - Thread-safe and re-entrant: any number of host threads may call concurrently (the reference's
 *     strategy is a stateless ZST, src/strategies/scalar.rs:11-20).  The only internal state is a
 *     mutex-protected pool of pipes (three streams + chunk buffers in device memory) used by the
 *     host-pointer entry points and the list of host ranges pinned through this library; device
 *     tables are immutable.
 *   - There is no CPU fallback: without a usable HIP device the calls fail with
 *     HADES252_ERR_NO_DEVICE / HADES252_ERR_HIP.
 */
#ifndef HADES252_H
#define HADES252_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HADES252_WIDTH 5              /* src/lib.rs:27 */
#define HADES252_TOTAL_FULL_ROUNDS 8  /* src/lib.rs:21 */
#define HADES252_PARTIAL_ROUNDS 59    /* src/lib.rs:25 */

#define HADES252_OK 0
#define HADES252_ERR_INVALID_ARG (-1)   /* NULL pointer with n > 0, bad round / index / device count */
#define HADES252_ERR_HIP (-2)           /* a HIP runtime call failed; see hades252_last_hip_error() */
#define HADES252_ERR_NOT_CANONICAL (-3) /* a canonical-bytes input encodes a value >= p */
#define HADES252_ERR_NO_DEVICE (-4)     /* no HIP device visible */
#define HADES252_ERR_SCRATCH (-5)       /* scratch buffer too small */
#define HADES252_ERR_OUT_OF_CONSTANTS (-6) /* cursor + WIDTH > 960: the reference panics with
                                              "Hades252 out of ARK constants" (src/strategies.rs:40) */

/* kernel selectors for hades252_perm_batch_dev_ex (all produce identical bits) */
#define HADES252_KERNEL_DEFAULT 0
#define HADES252_KERNEL_LITERAL 1 /* the reference's round structure, 1972 Montgomery products */
#define HADES252_KERNEL_FAST 2    /* scale-tracked small-integer MDS formulation, one state per lane:
                                     the throughput kernel */
#define HADES252_KERNEL_COOP 3    /* same arithmetic, the five words of a state on five waves: ~104 us per
                                     launch up to 16 384 states, ~45 % of the throughput of FAST */
#define HADES252_KERNEL_LANES 4   /* one state per wave, every field element spread over a 16-lane row: the
                                     lowest latency for ONE permutation -- the reference's own call shape
                                     (README.md:60-61): 50 us up to 768 states (helper wave per three states), 54-57 us up
                                     to 1 024 */
#define HADES252_KERNEL_ROWS 5    /* the same lane arithmetic, one state per 16-lane ROW, four per wave, the throughput
                                     kernel's schedule */
/* The size rule of HADES252_KERNEL_DEFAULT lives in ONE place, the library: hades252_kernel_for(n) is the selector
 * hades252_perm_batch_dev(.., n_perms = n, ..) runs (never DEFAULT, never LITERAL); hades252_chain_form_for(n) is the form
 * the chain entry points (sponge, streaming absorb, path verification, tree update) run for n chains, and a full Merkle
 * level for n parents (one of LANES, ROWS, COOP, FAST -- the per-state arithmetic of that kernel).  Two exceptions: a
 * ragged level of 4 097 .. 16 384 parents runs FAST (COOP takes full levels only), and a tree build or root may run
 * several full levels of arity 2 or 4 in one fused COOP launch (k_merkle_coop), the smaller ones included; hades252_kernel_name gives
 * the name of the __global__ function a profiler shows for a selector and batch size ("k_perm_fast", "k_perm_lanes", ..;
 * NULL for an unknown selector). */
int hades252_kernel_for(size_t n_perms);
int hades252_chain_form_for(size_t n_chains);
const char *hades252_kernel_name(int kernel, size_t n_perms);

/* ---- meta --------------------------------------------------------------------------- */
/* Strategy::rounds() (src/strategies.rs:160-162): TOTAL_FULL_ROUNDS + PARTIAL_ROUNDS = 67 */
int hades252_rounds(void);
int hades252_device_count(void);
const char *hades252_strerror(int code);
/* hipError_t of the most recent failing HIP call on this thread (0 if none) */
int hades252_last_hip_error(void);
const char *hades252_version(void);

/* ---- Strategy::perm, batched (src/strategies.rs:140-157 via ScalarStrategy) --------------
 * DELIBERATELY NOT EXPORTED: `hades252_perm_batch_cpu(uint64_t *, size_t, int n_threads)`, which SURVEY.md section 8(b)
 * lists as "the C++ oracle / baseline".  The product has no CPU path at all: a caller that wants the reference's CPU
 * behaviour keeps calling the reference's `ScalarStrategy` (that is what `HipStrategy` delegates the per-operation trait
 * methods to), and the C port that `bench.py` times as `cpu_baseline` lives under oracle/ as
 * test infrastructure -- linking it into this library would make every parity claim circular (the checker would ship
 * inside the thing it checks) and would let a missing GPU go unnoticed.  Do not "fix" this by linking oracle/ in:
 * tests/test_abi.py::test_no_cpu_fallback_in_product fails if anything under hades252_amd/, include/ or rust/ reaches
 * it.  For ONE permutation per call the CPU is the right tool anyway -- see the crossover table in INTEGRATION.md. */
/* In place on host memory, Montgomery limbs.  n_perms == 1 is exactly
 * `ScalarStrategy::new().perm(&mut state)` (README.md:60-61). */
int hades252_perm_batch(uint64_t *states, size_t n_perms);
/* In place on host memory, canonical bytes (5 x 32 B per state). */
int hades252_perm_batch_bytes(uint8_t *states, size_t n_perms);
/* In place on device memory, Montgomery limbs, asynchronous on `stream`. */
int hades252_perm_batch_dev(void *d_states, size_t n_perms, void *stream);
int hades252_perm_batch_dev_ex(void *d_states, size_t n_perms, void *stream, int kernel);
/* Host batch sharded over the first n_devices GPUs (contiguous ranges, one host thread and
 * pipe per device, no collective).  n_devices <= 0 means all visible devices.  A buffer the caller page-locked
 * (hades252_host_alloc / _register: portable, every device sees it) goes straight to DMA on every link; ordinary memory
 * travels through each worker's staging threads (3 + 3 CPU threads per worker). */
int hades252_perm_batch_multi(uint64_t *states, size_t n_perms, int n_devices);
/* Same with n_workers host threads; flags = HADES252_MULTI_VIRTUAL maps worker g to device g % (visible devices)
 * instead of device g, so that n_workers may exceed the device count (up to 64): a one-GPU box then runs the code
 * path of an 8-GPU node, several workers sharing a device.  Worker g owns states [n g / W, n (g+1) / W). */
#define HADES252_MULTI_VIRTUAL 1u
int hades252_perm_batch_multi_ex(uint64_t *states, size_t n_perms, int n_workers, unsigned flags);

/* ---- page-locked host memory for the host-pointer entry points ---------------------------------------
 * The reference's caller holds its states in ordinary memory (`&mut [BlsScalar]`, src/strategies.rs:140).  DMA needs
 * page-locked memory.  A caller with a long-lived buffer pins it ONCE: either allocate it here, or register an existing
 * allocation; hades252_perm_batch* recognise such memory (and memory the caller pinned through HIP itself) and go
 * straight to DMA (93-98 % of the link's bidirectional ceiling from 2^22 states on).  Anything else is never locked
 * when large: batches of more than 2^17 states travel through page-locked staging buffers of the library, filled and
 * drained by helper threads (HADES252_STAGE_THREADS per direction, default 3; ~88-92 % of the page-locked rate, at the
 * price of those CPU cores for the duration of the call); one-chunk batches of 8 MiB and more are page-locked in place
 * for the call; smaller ones are copied as pageable memory.  HADES252_HOST_PIN=0: plain pageable copies throughout.
 *   hades252_host_alloc      bytes of page-locked host memory, usable from every device; free with hades252_host_free
 *   hades252_host_register   page-lock [p, p + bytes) in place (any alignment); undo with hades252_host_unregister(p)
 *   hades252_host_is_pinned  1 if [p, p + bytes) is page-locked (by either call or through HIP), else 0
 * free / unregister return HADES252_ERR_INVALID_ARG for a pointer that did not come from alloc / register. */
int hades252_host_alloc(void **out, size_t bytes);
int hades252_host_free(void *p);
int hades252_host_register(void *p, size_t bytes);
int hades252_host_unregister(void *p);
int hades252_host_is_pinned(const void *p, size_t bytes);

/* ---- device memory for callers that do not link HIP themselves -----------------------------------------
 * A Rust crate binding only this library can keep its data resident and use every *_dev entry point through these:
 *   hades252_dev_alloc / _free   device memory on the current device (hipMalloc / hipFree)
 *   hades252_dev_upload          host -> device on `stream` (NULL = the default stream); asynchronous when the host memory
 *   hades252_dev_download        is page-locked (hades252_host_alloc / _register), device -> host likewise
 *   hades252_stream_create / _destroy / _sync    a stream handle for the `stream` arguments (sync(NULL) = the default one)
 * Pointers and streams are plain HIP objects: a HIP program may mix them with its own. */
int hades252_dev_alloc(void **d_ptr, size_t bytes);
int hades252_dev_free(void *d_ptr);
int hades252_dev_upload(void *d_dst, const void *h_src, size_t bytes, void *stream);
int hades252_dev_download(void *h_dst, const void *d_src, size_t bytes, void *stream);
int hades252_stream_create(void **stream);
int hades252_stream_destroy(void *stream);
int hades252_stream_sync(void *stream);

/* Optional.  Pays the one-time costs of the host-pointer path now instead of inside the first real call: loads the code
 * object (a one-state permutation on an internal buffer: ~35 ms in a fresh process) and, for n_perms_hint > 256, creates
 * the pipe a batch of that size would take -- streams, events, device chunk buffers, and the page-locked staging buffers
 * when the hint is large enough for the staging-thread path of ordinary memory -- and leaves it in the pool.  Current
 * device; a caller of the _multi entry points calls it once per device. */
int hades252_warm_up(size_t n_perms_hint);

/* ---- what the library caches, and how to give it back ---------------------------------------------------------
 * The host-pointer entry points reuse "pipes" (three streams, events, chunk buffers and a scratch arena in device memory,
 * a small page-locked staging buffer) so that a call pays no allocation.  The pool is bounded: per device it keeps at most
 * 16 pipes and at most HADES252_POOL_MAX_BYTES (environment, default 1 GiB) of device memory -- a pipe coming back from
 * a big one-shot call gives up its arena / chunk buffers first.  hades252_trim() destroys every pooled pipe (pipes in
 * use by concurrent calls are untouched and return to the pool later); hades252_pool_bytes() is the device memory the
 * pool holds right now on all devices.  A long-lived process that shares the GPU with another allocator calls trim after
 * a burst of large calls.  NOT counted by either figure: the page-locked HOST memory of the staging-thread path -- 120
 * MiB per pipe that has served a big call from ordinary memory; at most two such buffers stay cached per device (plus
 * one per call in flight) and a staging call reuses a pipe that owns one before allocating another; trim frees them. */
int hades252_trim(void);
size_t hades252_pool_bytes(void);
/* Helper threads per copy direction a host-pointer call on ORDINARY memory uses when it is one of n_workers concurrent
 * calls (the worker threads of the _multi entry points; 1 = a plain hades252_perm_batch): HADES252_STAGE_THREADS
 * (environment, 1 .. 6, default 3), capped so that n_workers x 2 directions x threads never exceeds the CPUs this process
 * may run on (sched_getaffinity), at least 1. */
int hades252_stage_threads(int n_workers);

/* ---- failure contract of the host-pointer entry points, and the hook that tests it -------------------------------
 * On HADES252_ERR_HIP from hades252_perm_batch* every 160-byte state of the caller's buffer holds EITHER its input OR
 * its permutation, never anything else (after a call of one chunk -- up to 65 536 states -- the buffer is either
 * untouched or completely written); which states were completed is unspecified: the call streams chunks in place, so making the whole batch atomic
 * would cost a second copy of it.  Every stream has drained when the call returns, nothing is leaked, the pipe is
 * destroyed rather than pooled, and the next call works.  hades252_merkle_root[_multi] write the root only on
 * success; a failing sponge call may already have delivered the digests of its first chunks.
 * Test hook: hades252_fault_inject("<site>:<nth>") makes the nth (1-based) HIP call of that class made by the
 * library from now on fail as if the runtime had refused it; sites: malloc, hostmalloc, hostregister, memcpy,
 * streamcreate, eventcreate, sync, worker (the device selection of one worker thread of the _multi entry points),
 * thread (the start of a helper thread: staging copies, _multi workers; reported as hipErrorOutOfMemory).
 * NULL or "" disarms.  The environment variable HADES252_FAIL_AT holds the same spec for processes that cannot call
 * the hook (read once, when the library is loaded: a static initialiser, so the variable must be set before dlopen /
 * process start).  Disarmed cost: one relaxed load per wrapped call.
 * HADES252_TEST_MAX_LAUNCH (tests only; read at the first call of hades252_perm_batch_dev*) lowers the number of states
 * one kernel launch of that entry point takes from 2^30, so that its multi-launch loop can be exercised on a few
 * thousand states; values below 256 are ignored. */
int hades252_fault_inject(const char *spec);

/* ---- the callers of perm, host memory in, host memory out -------------------------------------------------
 * One-shot forms of the Merkle root and the fixed-length sponge for data that lives in host memory (page-locked or not,
 * as for hades252_perm_batch: big inputs in ordinary memory go through the library's staging threads, nothing of the
 * caller's is page-locked): the leaves / messages travel to the device in chunks while the previous chunk is being
 * hashed (the first tree level / the sponge itself), only 32 bytes per tree / message travel back.
 *   hades252_merkle_root   leaves: n_leaves x 4 u64 (Montgomery limbs); pad: NULL or depth x 4 u64 (the padding table of
 *                          hades252_merkle_root_pad_dev, host memory); semantics of hades252_merkle_root_pad_dev
 *   hades252_sponge_hash   msgs: n_msgs x msg_len x 4 u64; digests: n_msgs x 4 u64; semantics of hades252_sponge_hash_dev */
int hades252_merkle_root(const uint64_t *leaves, size_t n_leaves, int arity, const uint64_t tag_mont[4], int out_idx,
                         const uint64_t *pad, uint64_t root[4]);
int hades252_sponge_hash(const uint64_t *msgs, size_t n_msgs, size_t msg_len, const uint64_t capacity_mont[4],
                         int pad_mode, uint64_t *digests);
/* The same root with the sub-trees of a FULL tree (n_leaves = arity^k) sharded over n_workers devices (0 = all), no
 * collective: worker g builds its complete sub-trees on device g, the sub-roots (32 B each) meet in host memory and one
 * more small tree finishes.  flags as hades252_perm_batch_multi_ex. */
int hades252_merkle_root_multi(const uint64_t *leaves, size_t n_leaves, int arity, const uint64_t tag_mont[4], int out_idx,
                               int n_workers, unsigned flags, uint64_t root[4]);
/* ... and the variable-length sponge (semantics of hades252_sponge_hash_var_ex_dev with sorting): scalars is the pool
 * (n_scalars x 4 u64), message i = scalars[offsets[i] .. offsets[i] + lengths[i]); *n_bad (may be NULL) receives the
 * number of messages that did not lie inside the pool (hashed as empty messages, never read). */
int hades252_sponge_hash_var(const uint64_t *scalars, size_t n_scalars, const uint64_t *offsets, const uint64_t *lengths,
                             size_t n_msgs, const uint64_t capacity_mont[4], int pad_mode, uint64_t *digests,
                             size_t *n_bad);

/* Per-round trace (witness pre-computation for GadgetStrategy, src/strategies/gadget.rs:41-133):
 * d_trace receives 67 batches, round-major: trace[r] (n_perms x 160 B, same AoS format) is the
 * state of every permutation after round r's mul_matrix; trace[66] equals the perm output.
 * d_states is not modified.  Needs 67 * 160 * n_perms bytes. */
int hades252_perm_trace_dev(const void *d_states, void *d_trace, size_t n_perms, void *stream);
/* kernel: HADES252_KERNEL_FAST (default; radix-2^29 rounds that hold every value in true form, so a round's five words
 * leave through an exact division by 32: ~200 M permutations/s) or HADES252_KERNEL_LITERAL (the reference's schedule,
 * ~35 M/s); identical bits. */
int hades252_perm_trace_dev_ex(const void *d_states, void *d_trace, size_t n_perms, void *stream, int kernel);

/* The same trace in SCALED form (opt-in, ~1.5x the rate: 313 against 215 M permutations/s at 2^20 states): trace[r] holds, fully reduced, the state the throughput kernel
 * carries after round r -- the true state times the running scale of the schedule, without the constants the partial rounds
 * defer -- so a word leaves the kernel without a multiplication.  The consumer recovers
 *     true[r][w] = scaled[r][w] * mul[r] + add[r][w]        (BlsScalar multiplication and addition, in-memory values)
 * with the 67 multipliers and 67 x 5 addends of hades252_perm_trace_scale_table (mul: 67 x 4 u64, add: 67 x 5 x 4 u64, host
 * memory, Montgomery limbs like every BlsScalar here; add[r] is zero in the full rounds) -- lazily, fused into whatever
 * reads the trace next.  Same layout and size as hades252_perm_trace_dev; d_states is not modified. */
int hades252_perm_trace_scaled_dev(const void *d_states, void *d_trace, size_t n_perms, void *stream);
int hades252_perm_trace_scale_table(uint64_t *mul, uint64_t *add);

/* Full gadget witness: every gate output GadgetStrategy assigns for a permutation (src/strategies/gadget.rs:41-133),
 * hades252_witness_wires() = 972 values per state in gate order:
 *   round 0: 5 x (w + c);  every round: per S-boxed word v^2, v^4, v^5 (5 words in a full round, the last word in a
 *   partial round), then for j = 0..4: r1[j] = M[j][0] v0 + M[j][1] v1 + M[j][2] v2 and
 *   r2[j] = M[j][3] v3 + M[j][4] v4 + r1[j] + (next round's constant j, 0 after the last round).
 * d_wires receives 972 batches, wire-major: wires[g] is n_perms scalars of 32 B (Montgomery limbs).  r2 of the last
 * round is the permutation's output.  Needs 972 * 32 * n_perms bytes; d_states is not modified.  ~125 M permutations/s at
 * 2^20 states (3.9 TB/s of wires written). */
int hades252_witness_wires(void);
int hades252_perm_witness_dev(const void *d_states, void *d_wires, size_t n_perms, void *stream);

/* ---- gadget witnesses of permutation chains: the sponge (f1) and Merkle openings (f2) ---- CONVENTION UNPINNED
 * The conventions are those of f1 and f2 below (capacity, padding, tag: parameters, still unpinned).  A batch of n chains
 * of S steps is S * n permutations, numbered rec = s * n + i (step-major, chain within the step):
 *   d_inputs receives S * n states of 160 B (the AoS format of the perm entry points): state rec enters permutation (s, i);
 *   d_wires  receives 972 * S * n scalars, wire-major, exactly as hades252_perm_witness_dev writes them.
 * Defining property: wires == hades252_perm_witness_dev(inputs) byte for byte, the S * n states taken as one flat batch.
 * The gadget's selection and add gates (which children, where the path node sits; the block added into words 1..4) are the
 * consumer's: the inputs carry their values.  A prover slices [972, S, n] per circuit.
 *
 * Sponge: the semantics of hades252_sponge_hash_dev (padding, the empty message, argument rules), S =
 * hades252_sponge_blocks(msg_len, pad_mode) (0 for an invalid pad_mode).  inputs[0][i] = [capacity, block 0];
 * inputs[s][i] = the output of permutation (s - 1, i) with block s added to words 1..4 (the absorb add gates' outputs).
 * d_digests (may be NULL) receives word 1 of the final state: hades252_sponge_hash_dev's digest.  One message per lane,
 * the state carried across its blocks: one message costs S x the latency of one perm_witness lane (no latency form).
 *
 * Merkle opening: the tree of hades252_merkle_build[_pad]_dev with the same arity, tag and pad (d_pad may be NULL, as
 * there), S = hades252_merkle_depth(n_leaves, arity).  inputs[l][q] = [tag, the arity children of the level-l group that
 * holds the level-l ancestor of leaf d_indices[q], 0 ...]: level 0 is the leaves, level l >= 1 comes from d_tree, a child
 * position past the end of its level reads pad[l] (zero without a table).  The permutations are independent: one gather
 * launch, then one perm_witness launch over all S * n_queries states.  An index >= n_leaves reads nothing outside the tree,
 * gets all-zero input states (and their wires) and increments *d_bad_count (device int, may be NULL).
 *
 * Rules (both): n = 0 is a no-op success (for the opening: after the tree shape is checked); d_inputs and d_wires must be
 * non-NULL and 16-byte aligned; S * n must be at most 2^30; besides those of hades252_sponge_hash_dev or
 * hades252_merkle_open_pad_dev (and a non-NULL tag, a 4-byte aligned d_bad_count).  All are checked before the device is
 * touched. */
size_t hades252_sponge_blocks(size_t msg_len, int pad_mode);
int hades252_sponge_witness_dev(const void *d_msgs, size_t n_msgs, size_t msg_len, const uint64_t capacity_mont[4],
                                int pad_mode, void *d_inputs, void *d_wires, void *d_digests, void *stream);
int hades252_merkle_open_witness_dev(const void *d_leaves, const void *d_tree, size_t n_leaves, int arity,
                                     const uint64_t tag_mont[4], const void *d_pad, const uint64_t *d_indices,
                                     size_t n_queries, void *d_inputs, void *d_wires, int *d_bad_count, void *stream);

/* ---- the trait's per-operation methods, batched on device ------------------------------- */
/* Strategy::add_round_key (src/strategies/scalar.rs:23-30).  The trait method takes the constants
 * ITERATOR (src/strategies.rs:33-41, :50-52); `cursor` is its position: word w of every state +=
 * ROUND_CONSTANTS[cursor + w].  Any 0 <= cursor <= 955 of the 960 constants (src/round_constants.rs:18)
 * is accepted; beyond that the reference panics "Hades252 out of ARK constants" and this returns
 * HADES252_ERR_OUT_OF_CONSTANTS.  The `round` forms are cursor = 5*round (what perm() does). */
int hades252_add_round_key_at_dev(void *d_states, size_t n_states, int cursor, void *stream);
int hades252_add_round_key_dev(void *d_states, size_t n_states, int round, void *stream);
/* Strategy::quintic_s_box (src/strategies/scalar.rs:32-34) on n_scalars independent scalars. */
int hades252_quintic_s_box_dev(void *d_scalars, size_t n_scalars, void *stream);
/* Strategy::mul_matrix (src/strategies/scalar.rs:36-49) on every state. */
int hades252_mul_matrix_dev(void *d_states, size_t n_states, void *stream);
/* Strategy::apply_full_round / apply_partial_round (src/strategies.rs:107-119, :79-93). */
int hades252_apply_full_round_dev(void *d_states, size_t n_states, int round, void *stream);
int hades252_apply_partial_round_dev(void *d_states, size_t n_states, int round, void *stream);
int hades252_apply_full_round_at_dev(void *d_states, size_t n_states, int cursor, void *stream);
int hades252_apply_partial_round_at_dev(void *d_states, size_t n_states, int cursor, void *stream);

/* ---- BlsScalar arithmetic, batched (external crate dusk-bls12_381; call sites src/strategies/scalar.rs:28,
 * :33, :44, src/round_constants.rs:41) ------------------------------------------------------------------
 * out[i] = a[i] op b[i] on Montgomery limbs (32 B each, fully reduced in and out; out may alias a or b).
 * op: 0 add, 1 mul, 2 square (b ignored), 3 from_raw (a = canonical limbs, b ignored), 4 reduce_signed (impl 1 only; a =
 *     the 256-bit two's-complement image of a signed integer x in (-p - 2^250, 2^250], b ignored; out = x mod p as plain
 *     limbs: the exit routine of the scaled per-round trace, exposed so that its rare branches can be driven directly).
 * impl: 0 = saturated 8 x u32 arithmetic of the literal kernels, 1 = radix-2^29 signed-limb arithmetic
 * of the shipped kernel.  Both give identical bits; tests regenerate the reference's constant blobs
 * through each of them. */
#define HADES252_FR_ADD 0
#define HADES252_FR_MUL 1
#define HADES252_FR_SQUARE 2
#define HADES252_FR_FROM_RAW 3
#define HADES252_FR_REDUCE_SIGNED 4
int hades252_fr_op_dev(int op, int impl, const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);

/* ---- wire format on device: BlsScalar::from_bytes / to_bytes ------------------------------ */
/* d_bad_count (device int, may be NULL) is incremented once per input >= p; such inputs
 * produce an all-zero scalar. */
int hades252_from_bytes_dev(const void *d_bytes, void *d_limbs, size_t n_scalars, int *d_bad_count, void *stream);
int hades252_to_bytes_dev(const void *d_limbs, void *d_bytes, size_t n_scalars, void *stream);

/* ---- Poseidon Merkle trees over the permutation (caller shape of dusk-poseidon, README.md:9) -------
 * parent = perm([tag, child_0 .. child_{arity-1}, 0 ..])[out_idx]; tag in Montgomery limbs.  The external convention
 * for arity 4 is tag = 2^4 - 1 = 15, out_idx = 1 (NOT pinned by the reference: both are parameters).  Digests are 32 B
 * Montgomery limbs.
 * Shapes: arity 2, 3 or 4 for trees (1 .. 4 for single levels and path verification); ANY number of leaves >= 2.
 *   Level l (l = 0: the leaves) has n_l nodes, n_{l+1} = ceil(n_l / arity), down to one root: hades252_merkle_depth
 *   levels above the leaves.  Padding rule: a child position past the end of level l holds pad[l], a table of `depth`
 *   digests in DEVICE memory the caller supplies to the _pad entry points (NULL = the zero scalar at every level);
 *   hades252_merkle_empty_digests_dev fills it with the roots of empty subtrees (pad[0] = e0, pad[l+1] = the parent of
 *   `arity` copies of pad[l]) -- the table an append-only tree uses.  Trees whose leaf count is a power of the arity
 *   never touch the table. */
int hades252_merkle_depth(size_t n_leaves, int arity);      /* -1: invalid (arity not 2..4, or fewer than 2 leaves) */
/* One level.  _dev: n_parents full parents from arity * n_parents children (arity 1 .. 4);
 * _pad_dev: n_children children -> ceil(n_children / arity) parents, missing children = the digest at d_pad (32 B). */
int hades252_merkle_level_dev(const void *d_children, void *d_parents, size_t n_parents, int arity,
                              const uint64_t tag_mont[4], int out_idx, void *stream);
int hades252_merkle_level_pad_dev(const void *d_children, size_t n_children, void *d_parents, int arity,
                                  const uint64_t tag_mont[4], int out_idx, const void *d_pad, void *stream);
/* Root only.  d_scratch needs hades252_merkle_scratch_bytes(n_leaves, arity) bytes (0 for a one-level tree;
 * d_scratch may then be NULL); the root (32 B) is written to d_root.  Levels of more than 16 384 parents run one
 * parent per lane; full levels of 1 025 .. 16 384 parents five waves per parent (arity 2 / 4 and power-of-arity levels:
 * 64 parents per workgroup through several levels in LDS); levels of at most 1 024 parents one parent per wave. */
size_t hades252_merkle_scratch_bytes(size_t n_leaves, int arity);
int hades252_merkle_root_dev(const void *d_leaves, size_t n_leaves, int arity, void *d_scratch, size_t scratch_bytes,
                             const uint64_t tag_mont[4], int out_idx, void *d_root, void *stream);
int hades252_merkle_root_pad_dev(const void *d_leaves, size_t n_leaves, int arity, void *d_scratch, size_t scratch_bytes,
                                 const uint64_t tag_mont[4], int out_idx, const void *d_pad, void *d_root, void *stream);
/* Whole tree, every level kept: d_tree (hades252_merkle_tree_bytes = 32 * (n_1 + n_2 + ... + 1) bytes; for
 * n_leaves = arity^k that is 32 * (n_leaves - 1) / (arity - 1)) receives level 1, then level 2, ... ; the root is its
 * last 32 bytes.  0 = invalid shape. */
size_t hades252_merkle_tree_bytes(size_t n_leaves, int arity);
int hades252_merkle_build_dev(const void *d_leaves, size_t n_leaves, int arity, const uint64_t tag_mont[4], int out_idx,
                              void *d_tree, void *stream);
int hades252_merkle_build_pad_dev(const void *d_leaves, size_t n_leaves, int arity, const uint64_t tag_mont[4], int out_idx,
                                  const void *d_pad, void *d_tree, void *stream);
/* The padding table of empty subtrees: d_pad[0] = e0, d_pad[l+1] = parent of `arity` copies of d_pad[l], l < depth - 1. */
int hades252_merkle_empty_digests_dev(int arity, int depth, const uint64_t e0_mont[4], const uint64_t tag_mont[4],
                                      int out_idx, void *d_pad, void *stream);
/* Openings (authentication paths) from a built tree: for query t with leaf index d_indices[t] (device u64) and
 * level l = 0 .. depth-1, the arity-1 siblings of the path node, in child order with the node's own position
 * (index / arity^l) % arity skipped: d_paths[t][l][s], 32 B each, depth * (arity-1) * 32 bytes per query; a sibling
 * position past the end of its level reads pad[l].  An index >= n_leaves yields an all-zero path (nothing outside the
 * tree is read). */
int hades252_merkle_open_dev(const void *d_leaves, const void *d_tree, size_t n_leaves, int arity,
                             const uint64_t *d_indices, size_t n_queries, void *d_paths, void *stream);
int hades252_merkle_open_pad_dev(const void *d_leaves, const void *d_tree, size_t n_leaves, int arity,
                                 const uint64_t *d_indices, size_t n_queries, const void *d_pad, void *d_paths,
                                 void *stream);
/* Batched path verification: d_roots[t] (32 B) = the root recomputed from leaf value d_leaves[t] (32 B each, query
 * order), its index d_indices[t] and its opening d_paths[t] (the layout above); the caller compares with the root it
 * trusts.  `depth` dependent permutations per query; arity 1 .. 4.  One query per lane; up to 1 024 queries one query per
 * WAVE (the low-latency form: 12 levels in 0.6 ms instead of 1.9), up to 4 096 four queries per wave (1.0 ms), up to 16 384 five
 * waves per query (1.3 ms). */
int hades252_merkle_verify_dev(const void *d_leaves, const uint64_t *d_indices, const void *d_paths, size_t n_queries,
                               int depth, int arity, const uint64_t tag_mont[4], int out_idx, void *d_roots, void *stream);
/* Incremental update (the append / overwrite path of a Merkle-tree caller: README.md:9 names the tree, the update is the
 * operation it serves): the caller has overwritten the leaves d_leaves[d_indices[q]], q < n_updates (device u64; sorted
 * lists do each ancestor once, any order is correct, an index >= n_leaves is ignored); their ancestors in d_tree -- built
 * by hades252_merkle_build[_pad]_dev with the same arity, tag, out_idx and pad -- are recomputed bottom-up in place:
 * at most depth * n_updates permutations, one launch per level, the form per level by hades252_chain_form_for (one
 * ancestor per wave for up to 1 024 updates: ~51 us a level).  A level with no more parents than updates is recomputed whole. */
int hades252_merkle_update_dev(const void *d_leaves, void *d_tree, size_t n_leaves, int arity, const uint64_t tag_mont[4],
                               int out_idx, const void *d_pad, const uint64_t *d_indices, size_t n_updates, void *stream);
/* Forest: n_trees independent trees of leaves_per_tree = arity^k leaves each (leaves contiguous, tree after tree); level l
 * of all trees is one launch; d_roots receives n_trees roots.  Scratch: hades252_merkle_forest_scratch_bytes. */
size_t hades252_merkle_forest_scratch_bytes(size_t n_trees, size_t leaves_per_tree, int arity);
int hades252_merkle_forest_dev(const void *d_leaves, size_t n_trees, size_t leaves_per_tree, int arity, void *d_scratch,
                               size_t scratch_bytes, const uint64_t tag_mont[4], int out_idx, void *d_roots, void *stream);
/* arity-4 forms (BASELINE config 4).  hades252_merkle4_scratch_bytes is 0 both for a one-level tree (4 leaves need no
 * scratch) and for an invalid shape: hades252_merkle_depth(n, 4) < 1 tells the second from the first. */
int hades252_merkle4_level_dev(const void *d_children, void *d_parents, size_t n_parents,
                               const uint64_t tag_mont[4], int out_idx, void *stream);
size_t hades252_merkle4_scratch_bytes(size_t n_leaves);
int hades252_merkle4_root_dev(const void *d_leaves, size_t n_leaves, void *d_scratch, size_t scratch_bytes,
                              const uint64_t tag_mont[4], int out_idx, void *d_root, void *stream);

/* ---- batched sponge (caller shape of dusk-poseidon's sponge hash, README.md:9) ----
 * d_msgs: n_msgs messages of msg_len scalars each (Montgomery limbs, contiguous: message i at scalar
 * offset i*msg_len).  state = [capacity, 0, 0, 0, 0]; each block of 4 scalars is added to words 1..4,
 * then permuted; pad_mode 1 first appends a single scalar 1 (then zeros), pad_mode 0 zero-fills;
 * at least one permutation is always applied.  Digest i = word 1 (32 B) -> d_digests[i].
 * dusk-poseidon is not part of the reference tree: capacity and padding are parameters and this
 * entry point's parity is pinned to this repo's oracle only.
 * A sponge is a chain of dependent permutations per message: batches of up to 1 024 messages (all sponge entry points,
 * hades252_sponge_absorb_dev included) run one message per WAVE on the low-latency arithmetic, ~50 us per block -- ONE
 * long message hashes at the speed of a CPU core (52 us per block) instead of 160 us per block; up to 4 096 four messages per
 * wave (~80 us per block), up to 16 384 five waves per message (~105 us); larger batches run one message per lane (throughput). */
int hades252_sponge_hash_dev(const void *d_msgs, size_t n_msgs, size_t msg_len, const uint64_t capacity_mont[4],
                             int pad_mode, void *d_digests, void *stream);
/* Variable-length batch: message i = d_scalars[d_offsets[i] .. d_offsets[i] + d_lengths[i]) (offsets and
 * lengths in scalars, device arrays of n_msgs u64; messages may overlap or leave gaps; length 0 allowed).
 * n_scalars = size of the pool: a message that does not lie inside it is never read -- it is hashed as the empty
 * message and d_bad_count (device int, may be NULL) is incremented.
 * Same absorption / padding rule per message as above (CONVENTION UNPINNED: parameters, see above).
 * Every lane of a wave runs to the longest message among the wave's 64.  _ex with d_scratch != NULL
 * (hades252_sponge_sort_scratch_bytes(n_msgs) bytes of device memory) first sorts the message indices by block count
 * on the device (three small launches), so that a wave's messages are alike: ragged batches keep > 90 % of the lanes
 * on useful permutations instead of ~50 %.  The digests are the same and land in message order either way. */
int hades252_sponge_hash_var_dev(const void *d_scalars, size_t n_scalars, const uint64_t *d_offsets,
                                 const uint64_t *d_lengths, size_t n_msgs, const uint64_t capacity_mont[4], int pad_mode,
                                 void *d_digests, int *d_bad_count, void *stream);
size_t hades252_sponge_sort_scratch_bytes(size_t n_msgs);
int hades252_sponge_hash_var_ex_dev(const void *d_scalars, size_t n_scalars, const uint64_t *d_offsets,
                                    const uint64_t *d_lengths, size_t n_msgs, const uint64_t capacity_mont[4], int pad_mode,
                                    void *d_digests, int *d_bad_count, void *d_scratch, size_t scratch_bytes, void *stream);
/* Streaming sponge: the states (160 B each, the AoS format of the perm entry points) live in device memory between
 * calls, so a caller can keep absorbing.  init: state = [capacity, 0, 0, 0, 0]; absorb: for t < blocks_each, words
 * 1..4 += d_blocks[i][t][0..3] (4 scalars = 128 B per block, state-major), then the permutation; squeeze: d_digests[i]
 * = word `word` of state i (dusk-poseidon's sponge returns word 1).  Padding is the caller's: the final block carries
 * whatever padding scalars the convention wants.  init + absorb of ceil(len / 4) zero-filled blocks + squeeze(1)
 * equals hades252_sponge_hash_dev with pad_mode 0. */
int hades252_sponge_init_dev(void *d_states, size_t n_states, const uint64_t capacity_mont[4], void *stream);
int hades252_sponge_absorb_dev(void *d_states, const void *d_blocks, size_t n_states, int blocks_each, void *stream);
int hades252_sponge_squeeze_dev(const void *d_states, void *d_digests, size_t n_states, int word, void *stream);
/* Named parameter sets a dusk-poseidon caller would pass -- NAMED, NOT PINNED: that crate is outside the reference
 * tree (README.md:9 only names it); the values below are the commonly described conventions, to be checked against
 * the crate version in use:
 *   "sponge/pad10"   capacity = 2^64 (Montgomery form), pad_mode 1 (a single 1, then zeros), digest = word 1
 *   "merkle/arity4"  tag = 2^4 - 1 = 15 in word 0, children in words 1..4, digest = word 1 */

/* ---- batched Poseidon cipher (caller shape of dusk-poseidon's PoseidonCipher, README.md:9) ---- CONVENTION UNPINNED
 * Authenticated encryption of n_msgs independent messages of msg_len scalars each (Montgomery limbs, as everywhere).
 * dusk-poseidon is not part of the reference tree: the construction is recalled from that crate (<= 0.33), the domain
 * word is a parameter and parity is pinned only to this repo's model (tests/cipher_model.py).  Per message, with key
 * (kx, ky) (the shared secret's affine coordinates), nonce n, M = msg_len and D = domain_mont:
 *   state = [D, M, kx, ky, n]   (M as the field element M)
 *   encrypt: for each block of 4 words: perm; words 1.. += the block's message words, which are also the cipher words;
 *            then perm; c[M] = word 1 (the tag).  M + 1 cipher words per message.
 *   decrypt: the same chain (message word = cipher word - state word, state word = cipher word); then perm;
 *            ok = (c[M] == word 1) and every cipher word canonical (< p); a rejected message comes out as M zeros.
 * The crate's instance is M = 2, D = 2^32 (Montgomery form); for M <= 4 the block count ceil(M / 4) is the crate's, for
 * larger M this is the natural generalisation.  Encrypt inputs must be canonical (not checked, as for perm).
 * Layouts (AoS, 32 B per scalar): messages n x M, keys n x 2, nonces n x 1, ciphers n x (M + 1), ok n bytes.
 * Rules: n_msgs = 0 is a no-op success; a NULL array with n_msgs > 0, msg_len 0 or > HADES252_CIPHER_MAX_LEN, a
 * scalar array that is not 16-byte aligned, d_rejected not 4-byte aligned or n_msgs > 2^30 is HADES252_ERR_INVALID_ARG,
 * all checked before the device is touched.  d_rejected (device int, may be NULL) is INCREMENTED by the number of
 * rejected messages.  Up to 1 024 messages run one per wave (latency: about 2 x 52 us at M = 2), more run one per lane.
 * Callers holding the 96-byte serialised form (three canonical 32-byte scalars) convert it with hades252_from_bytes_dev. */
#define HADES252_CIPHER_MAX_LEN 1024
/* dusk-poseidon's domain word 2^32 in the memory format (Montgomery limbs, least significant first), as an initialiser:
 * uint64_t dom[4] = HADES252_CIPHER_DOMAIN_MONT; */
#define HADES252_CIPHER_DOMAIN_MONT {0x355094eacaaf6b13ull, 0xf6b10cb369a568efull, 0xe2c926a640cc3869ull, 0x736a6d3bed269aadull}
int hades252_cipher_encrypt_dev(const void *d_msgs, const void *d_keys, const void *d_nonces, size_t n_msgs, size_t msg_len,
                                const uint64_t domain_mont[4], void *d_ciphers, void *stream);
int hades252_cipher_decrypt_dev(const void *d_ciphers, const void *d_keys, const void *d_nonces, size_t n_msgs,
                                size_t msg_len, const uint64_t domain_mont[4], void *d_msgs, uint8_t *d_ok, int *d_rejected,
                                void *stream);
/* The same on host memory (any n_msgs: chunked through a pooled pipe, device memory bounded; ordinary or page-locked
 * memory).  *n_rejected (may be NULL) receives the number of rejected messages. */
int hades252_cipher_encrypt(const uint64_t *msgs, const uint64_t *keys, const uint64_t *nonces, size_t n_msgs, size_t msg_len,
                            const uint64_t domain_mont[4], uint64_t *ciphers);
int hades252_cipher_decrypt(const uint64_t *ciphers, const uint64_t *keys, const uint64_t *nonces, size_t n_msgs,
                            size_t msg_len, const uint64_t domain_mont[4], uint64_t *msgs, uint8_t *ok, size_t *n_rejected);

/* ---- batched duplex sponge (the SAFE sponge of dusk-safe, which dusk-poseidon's hash, Merkle level and cipher use after
 * 0.33) ---- CONVENTION UNPINNED
 * n_msgs independent sponges that all follow one IO pattern: a list of absorb and squeeze calls fixed in advance, freely
 * interleaved, no padding.  Neither crate is part of the reference tree: the construction is recalled from dusk-safe /
 * dusk-poseidon and pinned only to this repository's model (tests/safe_model.py); how a tag is derived and which domain
 * separator a caller uses is theirs, so the tag is a parameter.  Rate 4, width 5, per sponge:
 *   state = [tag, 0, 0, 0, 0]; pos_absorb = 0; pos_squeeze = 0
 *   absorb(x_0 .. x_{n-1}):  for each x:  if pos_absorb == 4: state = perm(state); pos_absorb = 0
 *                                         state[1 + pos_absorb] += x;  pos_absorb += 1
 *                            afterwards:  pos_squeeze = 4                     (the next squeeze permutes first)
 *   squeeze(n):              n times:     if pos_squeeze == 4: state = perm(state); pos_squeeze = 0; pos_absorb = 0
 *                                         output state[1 + pos_squeeze];  pos_squeeze += 1
 * A call is one uint32_t: HADES252_SAFE_ABSORB (bit 31) set = absorb, the low 31 bits = its length (SAFE's own encoding).
 * A pattern is valid when it is not empty, starts with an absorb, ends with a squeeze, has no call of length 0, at most
 * HADES252_SAFE_MAX_CALLS calls and at most HADES252_SAFE_MAX_WORDS words in and as many out per sponge.  Consecutive
 * calls of one kind behave exactly like one call of the summed length.  Instances: [absorb(L), squeeze(1)] with tag c is
 * hades252_sponge_hash_dev(.., capacity c, pad_mode 0) in ceil(L / 4) permutations; [absorb(4), squeeze(1)] with tag 15 is
 * the arity-4 Merkle level; the crate's cipher is [absorb(2), absorb(1), squeeze(M), absorb(M), squeeze(1)] with cipher =
 * message + squeezed words, composed by the caller over the streaming calls below.
 * Layouts (AoS, 32 B per scalar, Montgomery limbs, canonical -- not checked, as for perm): d_in n_msgs x n_in words in call
 * order, d_out n_msgs x n_out words in call order, both message-major.
 * hades252_safe_pattern validates a pattern without touching a device and returns the words absorbed and squeezed per
 * sponge and the permutations per sponge (each pointer may be NULL).  hades252_safe_hash_dev runs the whole pattern in one
 * launch, asynchronous on `stream` (the pattern travels in the kernel arguments).  Up to 1 024 sponges run one per wave
 * (latency), more run one per lane; there is no four-per-wave or five-waves form: 1 025 .. 16 384 sponges run per lane.
 * Streaming, for callers whose next input depends on what they read: states are those of hades252_sponge_init_dev
 * (capacity = tag, 160 B each); the two positions live in a caller-owned *cursor (0 = fresh; opaque otherwise), one for
 * the whole batch.  The streaming calls do not know a pattern: any sequence is served, and any split of a pattern into
 * streaming calls gives the bytes of the one-shot call.  len is 1 .. HADES252_SAFE_MAX_WORDS.
 * Rules: n_msgs / n_states = 0 is a no-op success (the cursor stays); a NULL array, a scalar array that is not 16-byte
 * aligned, an invalid pattern, length or cursor value, or more than 2^30 sponges is HADES252_ERR_INVALID_ARG, all decided
 * before the device is touched; *cursor is written on success only. */
#define HADES252_SAFE_MAX_CALLS 64
#define HADES252_SAFE_MAX_WORDS 1048576
#define HADES252_SAFE_ABSORB 2147483648u
int hades252_safe_pattern(const uint32_t *calls, size_t n_calls, size_t *n_in, size_t *n_out, size_t *n_perms);
int hades252_safe_hash_dev(const void *d_in, size_t n_msgs, const uint32_t *calls, size_t n_calls, const uint64_t tag_mont[4],
                           void *d_out, void *stream);
int hades252_safe_absorb_dev(void *d_states, size_t n_states, const void *d_in, size_t len, uint32_t *cursor, void *stream);
int hades252_safe_squeeze_dev(void *d_states, size_t n_states, size_t len, void *d_out, uint32_t *cursor, void *stream);
/* The same on host memory (any n_msgs: chunked through a pooled pipe, device memory bounded; ordinary or page-locked
 * memory). */
int hades252_safe_hash(const uint64_t *in, size_t n_msgs, const uint32_t *calls, size_t n_calls, const uint64_t tag_mont[4],
                       uint64_t *out);

/* ---- gadget witnesses of the cipher (f5): the third chain of row f4 ---- CONVENTION UNPINNED
 * The construction of hades252_cipher_*_dev above (and of tests/cipher_model.py), recorded as the chain witnesses record the
 * sponge and Merkle openings: S = hades252_cipher_perms(M) = ceil(M / 4) + 1 permutations per message (0 for an invalid M),
 * record rec = s * n + i (step-major), d_inputs receives S * n states of 160 B, d_wires 972 planes of S * n scalars.
 *   inputs[0][i] = [D, M, kx, ky, nonce]   (M as the field element M, Montgomery form, as the cipher builds it)
 *   encrypt: inputs[s][i] (s >= 1) = the output of permutation (s - 1, i) with message word 4 (s - 1) + j added to word
 *            1 + j (the words that exist); these sums are the cipher words.
 *   decrypt: inputs[s][i] = the output of permutation (s - 1, i) with word 1 + j replaced by cipher word 4 (s - 1) + j
 *            REDUCED mod p (a 256-bit word is < 2.2 p), so every input state is canonical, accepted message or not.
 * Defining property: wires == hades252_perm_witness_dev(inputs) byte for byte, the S * n states taken as one flat batch.
 * Hence the decrypt witness of encrypt(m) is the encrypt witness of m, inputs and wires alike.  Word 1 of the final state
 * (the tag) is r2[1] of the last round of record (S - 1) n + i.
 * Side outputs, each may be NULL (not written): encrypt: d_ciphers (n x (M + 1)), byte for byte what
 * hades252_cipher_encrypt_dev writes; decrypt: d_msgs (n x M), d_ok (n bytes) and *d_rejected (incremented), byte for byte
 * what hades252_cipher_decrypt_dev gives (a wrong tag or a non-canonical cipher word: M zero words, ok = 0).
 * One message per lane, the state carried across its steps: one message costs S x the latency of one perm_witness lane.
 * Rules: those of hades252_cipher_*_dev (the side outputs optional) and of the chain witnesses: n_msgs = 0 is a no-op
 * success; d_inputs and d_wires must be non-NULL and 16-byte aligned; S * n_msgs must be at most 2^30.  All are checked
 * before the device is touched. */
size_t hades252_cipher_perms(size_t msg_len);
int hades252_cipher_encrypt_witness_dev(const void *d_msgs, const void *d_keys, const void *d_nonces, size_t n_msgs,
                                        size_t msg_len, const uint64_t domain_mont[4], void *d_inputs, void *d_wires,
                                        void *d_ciphers, void *stream);
int hades252_cipher_decrypt_witness_dev(const void *d_ciphers, const void *d_keys, const void *d_nonces, size_t n_msgs,
                                        size_t msg_len, const uint64_t domain_mont[4], void *d_inputs, void *d_wires,
                                        void *d_msgs, uint8_t *d_ok, int *d_rejected, void *stream);

/* ---- gadget witnesses of the duplex sponge (f9): the fourth chain of row f4, one-shot and streaming ---- CONVENTION UNPINNED
 * The construction of hades252_safe_*_dev above (and of tests/safe_model.py), recorded as the other chain witnesses are:
 * a batch of n sponges that run S permutations each is S * n records, rec = s * n + i (step-major); d_inputs receives S * n
 * states of 160 B, d_wires 972 planes of S * n scalars, wire-major.
 *   inputs[0][i] = [tag, 0, 0, 0, 0] with the words absorbed before the first permutation added at their positions;
 *   inputs[s][i] (s >= 1) = the output of permutation (s - 1, i) with the words absorbed between permutations s - 1 and s
 *   added at their positions.  Words squeezed in between are read, not changed: the gadget's add gates are the consumer's,
 *   the inputs carry their values.
 * Defining property: wires == hades252_perm_witness_dev(inputs) byte for byte, the S * n states taken as one flat batch.
 * The output of the last permutation is r2 of the last round of record (S - 1) n + i.
 * One-shot (hades252_safe_witness_dev): the whole IO pattern of hades252_safe_hash_dev, S = n_perms of
 * hades252_safe_pattern(calls) (a valid pattern has S >= 1).  d_out (n x n_out, may be NULL: not written) is byte for byte
 * what hades252_safe_hash_dev writes; d_in is not modified.
 * Streaming (hades252_safe_absorb_witness_dev / hades252_safe_squeeze_witness_dev): d_states, *cursor, d_in, d_out and len
 * mean exactly what they mean for hades252_safe_absorb_dev / hades252_safe_squeeze_dev, and after the call d_states, d_out
 * and *cursor hold exactly the bytes the plain call would have left.  d_inputs / d_wires are sized for total_steps steps
 * (plane length total_steps * n_states); the t-th permutation a call runs is step *step + t.  A call that runs q
 * permutations needs *step + q <= total_steps and adds q to *step on success only (q = 0 is legal: nothing is recorded).
 * Any split of a pattern into streaming witness calls with total_steps = the pattern's S gives the d_inputs, d_wires and
 * output bytes of the one-shot call.  The crate's cipher is composed over them as over the plain calls.
 * One sponge per lane whatever the batch size, the state carried across its steps: one sponge costs S x the latency of
 * one perm_witness lane; there is no one-per-wave latency form, as for the other chain witnesses.
 * Rules, all decided before the device is touched: those of the plain calls (n_msgs / n_states = 0 is a no-op success: the
 * cursor and the step stay), and d_inputs / d_wires non-NULL and 16-byte aligned, d_out of the one-shot call 16-byte
 * aligned when not NULL, step non-NULL, S * n_msgs (one-shot) or total_steps * n_states (streaming) at most 2^30,
 * *step + q <= total_steps.  Input words canonical and unchecked, as for hades252_safe_hash_dev. */
int hades252_safe_witness_dev(const void *d_in, size_t n_msgs, const uint32_t *calls, size_t n_calls,
                              const uint64_t tag_mont[4], void *d_inputs, void *d_wires, void *d_out, void *stream);
int hades252_safe_absorb_witness_dev(void *d_states, size_t n_states, const void *d_in, size_t len, uint32_t *cursor,
                                     void *d_inputs, void *d_wires, size_t total_steps, size_t *step, void *stream);
int hades252_safe_squeeze_witness_dev(void *d_states, size_t n_states, size_t len, void *d_out, uint32_t *cursor,
                                      void *d_inputs, void *d_wires, size_t total_steps, size_t *step, void *stream);

/* ---- batched proof-of-work grinding over the permutation (f10) ---- CONVENTION UNPINNED
 * The search a Fiat-Shamir grind, a rate-limiting puzzle or a proof of work over a Poseidon transcript needs: the smallest
 * nonce whose digest is below a target.  Nothing in the reference tree defines a proof of work: the definition is this
 * repository's own and pinned only to its model (tests/grind_model.py).  A job is a seed state of five scalars.  For a
 * nonce x < 2^64
 *   candidate(x) = the seed with word `word` replaced by seed[word] + x (mod p)
 *   digest(x)    = the canonical integer (what hades252_to_bytes_dev gives, NOT the Montgomery limbs) of word `out_idx` of
 *                  perm(candidate(x))
 *   x is a hit  <=>  digest(x) < target, strictly.  target is any 256-bit integer: 0 never hits, anything >= p hits at once.
 * The answer of job j is the SMALLEST hit in [first_nonce, first_nonce + max_nonces): found[j] = 1 and nonces[j] = that
 * nonce, or found[j] = 0 and nonces[j] left untouched.  It is a pure function of the arguments: it does not depend on grid
 * sizes, launch windows, early exits or dispatch order.  All jobs of a call share word, out_idx, target and the range.
 * In sponge terms (both sponges add an absorbed word into a rate word) a candidate is one absorb of x into word `word` of a
 * resident state, one permutation and one word read: hades252_sponge_absorb_dev / hades252_sponge_squeeze_dev verify a nonce.
 * Host memory in and out (a job is 160 bytes in and 9 out: there is no device-pointer form).  seeds: n_jobs x 5 x 4
 * Montgomery limbs, fully reduced (not checked, as for perm); target: 4 limbs, little-endian, the plain integer.  The
 * search runs in rounds of one launch each; after a round 8 bytes per job come back, and it stops when every job is found
 * or the range is exhausted.
 * Rules, all decided before the device is touched: n_jobs = 0 is a no-op success; a NULL seeds, target, nonces or found,
 * word or out_idx outside 0 .. 4, n_jobs > HADES252_GRIND_MAX_JOBS (the job is a grid dimension) or first_nonce + max_nonces
 * > 2^64 is HADES252_ERR_INVALID_ARG; max_nonces = 0 sets every found[j] = 0 and succeeds without a device. */
#define HADES252_GRIND_MAX_JOBS 65535
int hades252_grind(const uint64_t *seeds, size_t n_jobs, int word, int out_idx, const uint64_t target[4], uint64_t first_nonce,
                   uint64_t max_nonces, uint64_t *nonces, uint8_t *found);

/* ---- the inverse permutation and batched fifth roots (f11) ----
 * The permutation run backwards.  Not a convention of this repository's: every round of Strategy::perm
 * (src/strategies.rs:79-157) is a key addition, x -> x^5 on a field with gcd(5, p - 1) = 1 and an invertible Cauchy matrix,
 * so the inverse is determined by the reference: perm_inverse(perm(x)) == x and perm(perm_inverse(y)) == y for every
 * canonical state.  Uses: Hades as a keyed block permutation (decryption), delay functions of the Sloth / MinRoot kind (the
 * fifth root is the slow direction, the forward call checks it), cryptanalysis and test construction.
 *   hades252_perm_inverse_batch    n_perms states of 5 x 4 limbs, each replaced by its preimage
 *   hades252_perm_inverse_rounds   undoes rounds round_hi - 1, ..., round_lo of the reference's schedule (rounds 0 .. 3 and
 *                                  63 .. 66 are full): the input is the state after round round_hi - 1 (trace[round_hi - 1] of
 *                                  hades252_perm_trace_dev), the output the state after round round_lo - 1, or the permutation's
 *                                  input when round_lo = 0.  (HADES252_ROUNDS_TOTAL, 0) is hades252_perm_inverse_batch.  It
 *                                  localises a disagreement to a round.
 *   hades252_fifth_root_batch      n_scalars independent scalars, x -> x^D with D = 5^-1 mod (p - 1): the inverse of
 *                                  hades252_quintic_s_box_dev, 0 -> 0
 * Host memory, in place, synchronous, the in-memory format of hades252_perm_batch (Montgomery limbs, fully reduced, not
 * checked).  Any n: the call is chunked through a pooled pipe and holds two chunks of device memory.
 * There is no device-pointer form, no canonical-bytes form and no one-state-per-wave latency form: a state is 160 bytes each
 * way for about 17 forward permutations of arithmetic (99 fifth roots of 311 Montgomery products each, 67 dense 5 x 5 matrix
 * products), so the copies hide behind the kernel.  One state alone costs about 17 permutation latencies, roughly 1 ms: that
 * figure is not measured.
 * Rules, all decided before the device is touched: n = 0 is a no-op success, even with a NULL pointer; NULL with n > 0, a
 * pointer that is not 8-byte aligned, or a round range outside 0 <= round_lo <= round_hi <= HADES252_ROUNDS_TOTAL is
 * HADES252_ERR_INVALID_ARG; round_hi == round_lo is a no-op success. */
#define HADES252_ROUNDS_TOTAL 67
int hades252_perm_inverse_batch(uint64_t *states, size_t n_perms);
int hades252_perm_inverse_rounds(uint64_t *states, size_t n_perms, int round_hi, int round_lo);
int hades252_fifth_root_batch(uint64_t *scalars, size_t n_scalars);

/* ---- column-major matrix commitments: row hashes, tree and openings (f12) ---- CONVENTION UNPINNED
 * What a prover's trace, a batch of interpolated polynomials or a column-hashing sealer holds: a matrix of n_rows x n_cols
 * scalars stored column by column, each column one contiguous array ("plane") with one entry per row,
 *   scalar (r, c) = planes[(c * plane_stride + r) * 4 .. +4]          (4 Montgomery limbs, fully reduced, not checked).
 * Every row is hashed, the digests are put under a Merkle tree, and rows are opened with their paths -- without the caller
 * transposing anything.  Everything is defined through what the library already computes (the conventions are those of the
 * sponge f1 and the tree f2: capacity, padding and tag are parameters, still unpinned):
 *   leaf[r]   the digest hades252_sponge_hash gives for the message (M[r][0], ..., M[r][n_cols - 1]) with the same
 *             capacity_mont and pad_mode;
 *   the tree  byte for byte what hades252_merkle_build_pad_dev writes over those leaves: same level order, same padding
 *             rule, same `pad` table (depth digests, here in HOST memory; NULL = zeros); the root is its last 32 bytes;
 *   opening   of row r: the row itself, row-major (n_cols scalars), and its path in the layout of
 *             hades252_merkle_open_pad_dev; an index >= n_rows yields an all-zero row and path, as hades252_merkle_open_dev
 *             does (nothing outside the matrix or the tree is read).
 *   hades252_matrix_row_digests   the leaves only: n_rows x 32 bytes
 *   hades252_matrix_commit        digests, tree and root in one call; digests and tree may each be NULL (not wanted, nothing
 *                                 is written through them), root may not.  tree: hades252_merkle_tree_bytes(n_rows, arity)
 *                                 bytes.  The digests never visit the host between the hashing and the tree.
 *   hades252_matrix_open          openings from what commit returned (digests and tree both needed): a gather in plain host
 *                                 code that touches no device.  rows_out: n_queries x n_cols scalars; paths_out: n_queries x
 *                                 depth x (arity - 1) x 32 bytes, depth = hades252_merkle_depth(n_rows, arity).  Duplicate and
 *                                 unsorted indices are fine.
 *   hades252_matrix_verify        roots[t] = the root recomputed from opened row t (rows: n_queries x n_cols scalars,
 *                                 row-major), its index and its path; the caller compares with the committed root.
 * Host memory in and out, synchronous.  The rows travel in chunks of K rows (a multiple of 256; up to 128 MiB over all
 * columns and at most 2^18 rows), one 2-D copy per chunk into one of two device buffers, and chunk i + 1 is copied while
 * chunk i is hashed: device memory is two chunks, n_rows x 32 bytes of digests and the tree, whatever the matrix.  A chunk's
 * kernel takes one permutation latency per block of four columns however few rows it has, so a matrix of more than about 64
 * columns (fewer than 2^16 rows per chunk) is bound by that latency, not by the link; the streaming form (f13, below) takes
 * such a matrix in column groups over all rows and is not.  Page-locked planes
 * (hades252_host_alloc / hades252_host_register) are recommended: from pageable memory the 2-D copies do not overlap the
 * kernel.
 * There is no device-pointer form (a block of a row is 128 bytes in for one permutation, against 160 in and 160 out for
 * hades252_perm_batch, so the copies are expected to hide behind the kernel), no canonical-bytes form, no witness form, and
 * only one kernel form, one row per lane: a matrix of a few hundred rows pays one permutation latency (about 160 us) per
 * block of four columns; there is no one-row-per-wave latency form.  hades252_matrix_verify does use the latency forms of
 * hades252_sponge_hash_dev and hades252_merkle_verify_dev for small batches of queries.
 * Rules, all decided before the device is touched: n_rows = 0 is a no-op success for hades252_matrix_row_digests and
 * n_queries = 0 for hades252_matrix_open and hades252_matrix_verify, even with NULL pointers; a NULL pointer that is needed
 * (planes, capacity_mont, tag_mont, root, indices, the outputs of row_digests / open / verify, digests and tree for open),
 * a pointer that is not 8-byte aligned, n_cols outside 1 .. HADES252_MATRIX_MAX_COLS, plane_stride < n_rows, pad_mode other
 * than 0 or 1, arity outside 2 .. 4, out_idx outside 0 .. 4, n_rows < 2 for commit and open (hades252_merkle_depth is -1),
 * n_rows or n_queries above 2^30, a depth outside 1 .. 64 for verify, or a byte count that overflows size_t is
 * HADES252_ERR_INVALID_ARG.  No device: HADES252_ERR_NO_DEVICE (there is no CPU fallback; hades252_matrix_open needs none). */
#define HADES252_MATRIX_MAX_COLS 4096      /* so the smallest chunk (256 rows) is 32 MiB */
int hades252_matrix_row_digests(const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride,
                                const uint64_t capacity_mont[4], int pad_mode, uint64_t *digests);
int hades252_matrix_commit(const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride,
                           const uint64_t capacity_mont[4], int pad_mode, int arity, const uint64_t tag_mont[4], int out_idx,
                           const uint64_t *pad, uint64_t *digests, uint64_t *tree, uint64_t root[4]);
int hades252_matrix_open(const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride, const uint64_t *digests,
                         const uint64_t *tree, int arity, const uint64_t *pad, const uint64_t *indices, size_t n_queries,
                         uint64_t *rows_out, uint64_t *paths_out);
int hades252_matrix_verify(const uint64_t *rows, size_t n_cols, const uint64_t *indices, const uint64_t *paths, size_t n_queries,
                           int depth, int arity, const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                           int out_idx, uint64_t *roots);

/* ---- streaming matrix commitments: column groups, resident row states (f13) ---- CONVENTION UNPINNED
 * The commitment of f12 for a matrix that is produced a group of columns at a time and may never be in host memory at once
 * (a trace and its low-degree extension, batches of interpolated polynomials): a stream is opened for n_rows rows, fed any
 * number of columns per call and finished at any point.  The row sponges stay on the device between the calls.
 * Everything is defined through f12.  After absorbs of g_1, ..., g_k columns let M be the n_rows x (g_1 + ... + g_k) matrix
 * of those columns in order:
 *   hades252_matstream_open      a stream for n_rows rows with this capacity word; *out is the handle (NULL on any failure).
 *                                It owns 160 bytes of device memory per row and, from the first digests / commit on, n_rows x
 *                                32 bytes of digests and the tree.  hades252_trim does not free what an open stream holds.
 *   hades252_matstream_absorb    the next n_cols columns, every row: scalar (r, j) of the group = planes[(j * plane_stride + r)
 *                                * 4 .. +4], layout and rules of f12, each call with its own planes and plane_stride.
 *                                Synchronous: the caller may reuse planes when it returns.
 *   hades252_matstream_cols      the number of columns absorbed so far
 *   hades252_matstream_digests   writes what hades252_matrix_row_digests(M, ..., pad_mode) writes
 *   hades252_matstream_commit    writes what hades252_matrix_commit(M, ...) writes: same digests, tree and root, same `pad`
 *                                table (depth digests in HOST memory; NULL = zeros); digests and tree may each be NULL, root
 *                                may not.  The digests never visit the host between the hashing and the tree.
 *   hades252_matstream_close     frees the stream; close(NULL) is a no-op success.
 * The padding is chosen at the end, not at open: it happens only there.  digests and commit are NON-DESTRUCTIVE -- they pad
 * and finish a copy of the state -- so the stream can go on absorbing afterwards and a caller may commit to every prefix.
 * State per row after c columns: the five-word sponge state with floor(c / 4) blocks added into words 1..4 and permuted and
 * the c % 4 columns of the open block added and not permuted.  Finish: under pad_mode 1 Montgomery one is added into word
 * 1 + c % 4; a permutation if c % 4 != 0 or pad_mode == 1; the digest is word 1 (hades252_sponge_blocks(c, pad_mode)
 * permutations in all).
 * A group travels in tiles of K rows x G columns (K = all rows up to 2^18, G = 128 MiB / (32 K) columns, a multiple of
 * four), one 2-D copy per tile into one of two device buffers, tile t + 1 copied while tile t is absorbed: a wide matrix
 * runs as full-device launches of a few blocks each, where hades252_matrix_commit (whose chunk holds all columns, hence
 * few rows) pays one permutation latency per block of four columns and chunk: 2^16 rows x 1 024 columns take 52 ms against
 * 738 ms (one MI355X, profiles/f13_matrix_stream/), and what is left is the chain of dependent permutations of a row.  A
 * call that is a single tile cannot overlap its copy with its kernel: feed several tiles per call where possible.  The
 * stream pays 320 bytes of device traffic per row and launch for its state, so a narrow matrix that is in memory anyway
 * gains nothing.  Page-locked planes are recommended, as for f12.
 * Host pointers only, like f10 to f12: no device-pointer form, no canonical-bytes form, no witness form, no latency form,
 * no openings (hades252_matrix_open gathers rows from whatever planes the caller still holds, a group at a time).
 * A stream is used by one thread at a time and with the device current that was current at open (with another one the
 * call is HADES252_ERR_INVALID_ARG); different streams, and streams alongside any other call of the library, are independent.
 * Rules, all decided before the device is touched.  open: out or capacity_mont NULL, n_rows 0 or above 2^30 is
 * HADES252_ERR_INVALID_ARG; no device is HADES252_ERR_NO_DEVICE.  Every other call with a NULL stream is
 * HADES252_ERR_INVALID_ARG, except close.  absorb: n_cols = 0 is a no-op success, even with NULL planes; NULL planes or
 * planes that are not 8-byte aligned, plane_stride < n_rows, a byte count that overflows size_t or a column total that
 * overflows uint64_t is HADES252_ERR_INVALID_ARG; there is no cap on the number of columns, per call or in total.  digests
 * and commit: no column absorbed so far, pad_mode other than 0 or 1, a NULL or misaligned output that is needed is
 * HADES252_ERR_INVALID_ARG; commit applies the rules of hades252_matrix_commit besides (n_rows >= 2, arity 2 .. 4, out_idx
 * 0 .. 4, tag_mont and root not NULL, 8-byte alignment).  An HADES252_ERR_INVALID_ARG leaves the stream exactly as it was.
 * A HIP failure inside a call returns HADES252_ERR_HIP and poisons the stream: every later absorb, digests or commit
 * returns HADES252_ERR_HIP without touching the device, cols still answers with the last good total, close always works. */
int hades252_matstream_open(void **out, size_t n_rows, const uint64_t capacity_mont[4]);
int hades252_matstream_absorb(void *ms, const uint64_t *planes, size_t n_cols, size_t plane_stride);
int hades252_matstream_cols(const void *ms, uint64_t *n_cols_so_far);
int hades252_matstream_digests(void *ms, int pad_mode, uint64_t *digests);
int hades252_matstream_commit(void *ms, int pad_mode, int arity, const uint64_t tag_mont[4], int out_idx, const uint64_t *pad,
                              uint64_t *digests, uint64_t *tree, uint64_t root[4]);
int hades252_matstream_close(void *ms);

/* ---- mixed-height matrix commitments: one root, fused batch verification (f14) ---- CONVENTION UNPINNED
 * A prover holds several matrices of different heights (a trace, its extension, quotient and lookup tables) and answers every
 * query index in all of them.  Instead of one tree, one root and one path per matrix (f12 / f13), ONE tree sits over the
 * tallest matrix, and the row digests of each shorter matrix are hashed into the level whose size equals its height: one
 * root, one path per query.  Everything is defined through what the library already computes (capacity, padding and the
 * two tags are parameters, still unpinned).  With a the arity (2 .. 4):
 *   groups    G <= HADES252_MMCS_MAX_GROUPS groups of heights h_0 > h_1 > ... > h_{G-1}, each h_g = a^(d_g), D = d_0 >= 1.  A
 *             group is every column absorbed for that height, in the order of the calls: an h_g x c_g matrix M_g.
 *   leaf_g[r] what hades252_matrix_row_digests gives for row r of M_g with the commitment's capacity_mont and the commit's
 *             pad_mode.
 *   nodes     node_D[i] = leaf_0[i].  For l = D - 1 .. 0: node_l[i] is the parent hades252_merkle_level_dev gives for the
 *             children node_{l+1}[a i .. a i + a - 1] with tag_mont and out_idx; if a group has d_g = l the node is then
 *             replaced by perm([inject_tag, node_l[i], leaf_g[i], 0, 0])[out_idx] -- the parent hades252_merkle_level_dev
 *             gives at arity 2 for the pair (node_l[i], leaf_g[i]) with tag = inject_tag_mont.  root = node_0[0].
 *   tree      node_D, then node_{D-1}, ..., then the root: final values, after injection.  hades252_mmcs_tree_bytes(h_0, a)
 *             = 32 (a^D + ... + a + 1), or 0 for an invalid shape (max_rows not a power of the arity, below the arity or
 *             above 2^30).
 *   opening   of index i < h_0: for every group its row i / (h_0 / h_g), which the caller gathers from its own planes, and
 *             ONE path: exactly what hades252_merkle_open_dev writes for d_leaves = node_D, d_tree = the rest, n_leaves =
 *             h_0 (D x (a - 1) siblings of 32 bytes).  An index >= h_0 yields an all-zero path.
 * With one group the tree is that group's digests followed by the tree of hades252_matstream_commit, and the root is the same.
 *   hades252_mmcs_new         a commitment with this capacity word; *out is the handle (NULL on any failure).
 *   hades252_mmcs_absorb      the next n_cols columns of the group of height n_rows, layout and rules of
 *                             hades252_matstream_absorb.  The group is created at first use: 160 bytes of state and 32 of
 *                             digest per row on the device (hades252_trim does not free them).  Calls for different heights
 *                             interleave freely.  Synchronous: the caller may reuse planes when it returns.
 *   hades252_mmcs_cols        the columns absorbed so far for that height; 0: no such group.
 *   hades252_mmcs_commit      NON-DESTRUCTIVE: every prefix can be committed and absorbing goes on.  tree
 *                             (hades252_mmcs_tree_bytes(h_0, arity) bytes) may be NULL, root may not; the root is written on
 *                             success only.  The digests never visit the host.
 *   hades252_mmcs_free        frees the commitment; free(NULL) succeeds.
 *   hades252_mmcs_open        paths from the tree commit returned: a plain host gather, no device.  paths_out: n_queries x D
 *                             x (arity - 1) x 32 bytes.  Duplicate and unsorted indices are fine.
 *   hades252_mmcs_verify      roots[t] = the root recomputed from opening t; the caller compares it with the root it trusts.
 *                             rows is query-major: query t holds the opened rows of all groups concatenated, tallest first,
 *                             cols[0] + ... + cols[n_groups - 1] scalars; paths as hades252_mmcs_open writes them.  Indices
 *                             are not range-checked, as in hades252_merkle_verify_dev.
 * Verification is ONE launch per chunk: lane t runs the whole chain of query t -- for each group the sponge blocks of its
 * row (hades252_sponge_blocks(cols[g], pad_mode)), the injection (g > 0), the levels up to the next group's height --
 * hades252_sponge_blocks summed over the groups + D + (G - 1) dependent permutations, where composing the existing calls
 * takes a sponge launch per group and a verify launch per tree segment.  The queries travel in chunks of at most 2^18
 * queries and 128 MiB of rows plus paths through two device buffers, chunk i + 1 copied while chunk i runs.  Commit runs
 * the groups' finishing launches one after the other, then one launch per level down to the shortest group's (each picks its
 * latency form by size), an injection launch where a group sits, and one tree build above.  Page-locked planes are
 * recommended, as for f12.
 * Host pointers only, like f10 to f13: no device-pointer form, no canonical-bytes form, no witness form, no latency form of
 * the verification, no multiproofs, no row gather (the caller holds the planes).
 * A commitment is used by one thread at a time and with the device current that was current at new (with another one the
 * call is HADES252_ERR_INVALID_ARG); different commitments, and commitments alongside any other call of the library, are
 * independent.
 * Rules, all decided before the device is touched.  new: out or capacity_mont NULL is HADES252_ERR_INVALID_ARG; no device is
 * HADES252_ERR_NO_DEVICE.  Every other call with a NULL handle is HADES252_ERR_INVALID_ARG, except free.  absorb: n_cols = 0
 * is a no-op success, even with NULL planes, and creates nothing; n_rows outside 1 .. 2^30, NULL planes or planes that are
 * not 8-byte aligned, plane_stride < n_rows, a byte count that overflows size_t, a column total that overflows uint64_t or
 * a 33rd distinct height is HADES252_ERR_INVALID_ARG and allocates nothing.  commit: pad_mode other than 0 or 1, arity
 * outside 2 .. 4, out_idx outside 0 .. 4, tag_mont, inject_tag_mont or root NULL, tree or root not 8-byte aligned, no group,
 * a height that is not a power of the arity or a tallest height below the arity is HADES252_ERR_INVALID_ARG and leaves the
 * handle exactly as it was.  open and verify: n_queries = 0 is a no-op success, even with NULL pointers; a NULL or
 * misaligned pointer, an invalid shape (open: hades252_mmcs_tree_bytes is 0; verify: n_groups outside 1 .. 32, heights that
 * are not strictly decreasing powers of the arity with heights[0] >= arity, cols[g] outside 1 .. 2^30), n_queries above 2^30
 * for verify or a byte count that overflows size_t is HADES252_ERR_INVALID_ARG.
 * A HIP failure inside a call returns HADES252_ERR_HIP and poisons the handle: every later absorb or commit returns
 * HADES252_ERR_HIP without touching the device, cols still answers with the last good totals, free always works. */
#define HADES252_MMCS_MAX_GROUPS 32
int hades252_mmcs_new(void **out, const uint64_t capacity_mont[4]);
int hades252_mmcs_absorb(void *mc, const uint64_t *planes, size_t n_rows, size_t n_cols, size_t plane_stride);
int hades252_mmcs_cols(const void *mc, size_t n_rows, uint64_t *n_cols_so_far);
int hades252_mmcs_commit(void *mc, int pad_mode, int arity, const uint64_t tag_mont[4], const uint64_t inject_tag_mont[4],
                         int out_idx, uint64_t *tree, uint64_t root[4]);
int hades252_mmcs_free(void *mc);
size_t hades252_mmcs_tree_bytes(size_t max_rows, int arity);
int hades252_mmcs_open(const uint64_t *tree, size_t max_rows, int arity, const uint64_t *indices, size_t n_queries,
                       uint64_t *paths_out);
int hades252_mmcs_verify(const uint64_t *rows, const uint64_t *heights, const uint64_t *cols, size_t n_groups,
                         const uint64_t *indices, const uint64_t *paths, size_t n_queries, int arity,
                         const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                         const uint64_t inject_tag_mont[4], int out_idx, uint64_t *roots);

/* ---- device-resident mixed-height commitments: absorb, open and verify on the device (f15) ---- CONVENTION UNPINNED
 * The commitment of f14, above, for a prover whose matrices already live in DEVICE memory: the same handle
 * (hades252_mmcs_new), the same groups, tree, openings and roots, byte for byte, without a copy to the host and back.  The
 * family is hades252_dmmcs_* ("d" for device-resident); hades252_mmcs_commit and hades252_mmcs_free stay the commit and the
 * free, and one handle may be fed through hades252_mmcs_absorb and hades252_dmmcs_absorb in any mixture.  The last argument
 * of absorb, open and verify is the caller's stream, as in every _dev call: the call enqueues there and returns; nothing is
 * synchronised and nothing is downloaded.  Device pointers are 16-byte aligned; the arrays that describe the parts
 * (d_planes, n_rows, n_cols, plane_strides, heights, cols) are HOST arrays and are not referenced after the call returns.
 *   hades252_dmmcs_absorb   n_parts = 1 .. HADES252_MMCS_MAX_GROUPS parts.  Part p is a column-major device matrix, scalar
 *                           (r, j) at d_planes[p] + (j * plane_strides[p] + r) * 32, absorbed as the next n_cols[p] columns
 *                           of the group of height n_rows[p], by the rules of hades252_mmcs_absorb per part: the group is
 *                           created at first use (its state planes are allocated and initialised before the call returns),
 *                           a 33rd distinct height is refused, a part with n_cols[p] = 0 is skipped whatever else it
 *                           holds.  The heights of one call are distinct.  All parts run as ONE launch: the grid is the
 *                           blocks of all parts laid end to end, shortest part first, so the short groups' chains of
 *                           permutations run beside the tall group's, not after it.  The column totals
 *                           (hades252_mmcs_cols) move at enqueue time.  The planes are only read, and may be reused once
 *                           the stream has passed the call.
 *   hades252_dmmcs_tree     the device tree of the last successful hades252_mmcs_commit, in the layout of f14 (*tree_bytes
 *                           = hades252_mmcs_tree_bytes(h_0, *arity); the root is its last 32 bytes), valid until the next
 *                           commit or free: a device prover can hand it to hades252_merkle_open_dev and friends itself
 *                           (d_leaves = the tree, d_tree = what follows its first h_0 digests).  No stream: nothing is enqueued.
 *   hades252_dmmcs_open     the openings of n_queries device indices from that tree.  The handle keeps no matrix, only
 *                           sponge states, so the caller passes the committed matrices in, tallest first, as absorb takes
 *                           them: strictly falling heights, every one a group of the handle, the first the height h_0 of
 *                           the committed tree.  d_rows: n_queries x (n_cols[0] + ... ) scalars, query-major, group g's row
 *                           index / (h_0 / h_g), the groups concatenated tallest first; d_paths: n_queries x D x (arity - 1)
 *                           digests, the paths of ONE call of hades252_merkle_open_dev on the tree -- exactly what
 *                           hades252_mmcs_verify and hades252_dmmcs_verify read.  An index >= h_0 gives an all-zero row
 *                           and an all-zero path: nothing outside the matrices and the tree is read.  Duplicate and
 *                           unsorted indices are fine.  Two launches: the row gather and the paths.
 *   hades252_dmmcs_verify   hades252_mmcs_verify with rows, indices, paths and roots in device memory (heights and cols
 *                           stay host arrays, the shape rules are the same): ONE launch over all n_queries <= 2^30
 *                           openings, straight from the caller's buffers -- no chunks, no staging buffer, no copy.
 * Ordering rule.  The library orders NOTHING between a caller's stream and its own streams, on which the host-form calls of
 * f14 run.  All hades252_dmmcs_* calls on one handle go on one stream, or the caller orders them; before any host-form call
 * on that handle (hades252_mmcs_absorb, hades252_mmcs_commit, hades252_mmcs_free) the caller synchronises that stream.  The
 * host-form calls are synchronous, so a hades252_dmmcs_* call enqueued after one returns sees its result.
 * Rules, all decided before the device is touched; a refused call leaves the handle exactly as it was.  A NULL handle, a NULL
 * array or output, n_parts outside 1 .. 32 is HADES252_ERR_INVALID_ARG.  absorb, per part with n_cols[p] > 0: n_rows[p]
 * outside 1 .. 2^30, a NULL or misaligned d_planes[p], plane_strides[p] < n_rows[p], a byte count that overflows size_t, a
 * column total that overflows uint64_t, a height that occurs twice in the call or a 33rd distinct height is
 * HADES252_ERR_INVALID_ARG; a call whose parts are all skipped is a no-op success.  tree and open: no successful commit yet
 * is HADES252_ERR_INVALID_ARG.  open: n_queries = 0 is a no-op success; n_rows[0] other than h_0, heights that do not fall
 * strictly, a height that is no group of the handle, n_cols[p] outside 1 .. 2^30, the plane rules of absorb, a misaligned
 * d_indices, d_rows or d_paths, n_queries x n_cols[p] above 2^30 or n_queries x D x (arity - 1) above 2^29 is
 * HADES252_ERR_INVALID_ARG.  verify: the rules of hades252_mmcs_verify, with 16-byte alignment for d_rows, d_paths, d_roots.
 * A handle is used with the device current that was current at new.  A launch that fails returns HADES252_ERR_HIP and
 * poisons the handle, as in f14 (verify has no handle to poison).
 * No witness form, no multiproofs, no device form of f12 / f13 on their own: one group of a commitment is that stream. */
int hades252_dmmcs_absorb(void *mc, const void *const *d_planes, const uint64_t *n_rows, const uint64_t *n_cols,
                          const uint64_t *plane_strides, size_t n_parts, void *stream);
int hades252_dmmcs_tree(const void *mc, const void **d_tree, size_t *tree_bytes, int *arity);
int hades252_dmmcs_open(const void *mc, const void *const *d_planes, const uint64_t *n_rows, const uint64_t *n_cols,
                        const uint64_t *plane_strides, size_t n_parts, const uint64_t *d_indices, size_t n_queries,
                        void *d_rows, void *d_paths, void *stream);
int hades252_dmmcs_verify(const void *d_rows, const uint64_t *heights, const uint64_t *cols, size_t n_groups,
                          const uint64_t *d_indices, const void *d_paths, size_t n_queries, int arity,
                          const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                          const uint64_t inject_tag_mont[4], int out_idx, void *d_roots, void *stream);

/* ---- row-major matrices for mixed-height commitments, host and device (f16) ---- CONVENTION UNPINNED
 * The commitments of f14 / f15, above, for a prover that keeps its matrices ROW by row (a trace is an array of rows, an opened
 * row a contiguous slice): the same handle (hades252_mmcs_new), groups, commit, tree, paths and verification, with no
 * transpose anywhere.  A ROW-MAJOR PART is an n_rows x n_cols matrix whose scalar (r, j) is at base + (r * stride + j) * 32
 * bytes, stride >= n_cols counted in scalars, every scalar four Montgomery limbs, fully reduced and not checked, as
 * everywhere.  Absorbing it into the group of height n_rows is DEFINED as absorbing the column-major matrix with the same
 * entries by the rules of hades252_mmcs_absorb: the handle then holds, byte for byte, the states it would hold after
 * hades252_mmcs_absorb / hades252_dmmcs_absorb of the transposed matrix, so commit, tree, paths, verification and roots are
 * what they were.  The group is created at first use, the open block position is the group's column total mod 4, and calls in
 * either layout, host and device, mix freely on one handle and one group (under the ordering rule of f15).  The family is
 * hades252_rmmcs_* ("r" for row-major, as f15's "d" is for device-resident): the hades252_mmcs_* and hades252_dmmcs_*
 * families stay exactly the calls of f14 and f15.
 *   HADES252_LAYOUT_COLS     column-major: strides[p] is the plane stride (rows per plane), scalar (r, j) at
 *                            d_mats[p] + (j * strides[p] + r) * 32.
 *   HADES252_LAYOUT_ROWS     row-major: strides[p] is the row stride (scalars per row).
 *   hades252_rmmcs_absorb_rows  the host form: the next n_cols columns of the group of height n_rows from a row-major matrix
 *                            in HOST memory, by the rules of hades252_mmcs_absorb.  Synchronous: the caller may reuse rows
 *                            when it returns.  The matrix travels in tiles of K rows x G columns through two device
 *                            buffers, tile t + 1 copied while tile t is absorbed, K and G as in hades252_matstream_absorb
 *                            (K = all rows up to 2^18, G = 128 MiB / (32 K) columns, a multiple of four): one pitched 2-D
 *                            copy per tile (source pitch row_stride * 32, width G * 32, height K), which is one contiguous
 *                            copy when a tile holds whole rows and row_stride = n_cols.  The tile lands row-major on the
 *                            device and is absorbed as it lies.  Page-locked rows are recommended, as for f12.
 *                            hades252_mmcs_open needs no twin: the caller gathers its own rows.
 *   hades252_rmmcs_absorb_ex hades252_dmmcs_absorb in every rule, with a layout per part: layouts is a HOST array, not
 *                            referenced after the call returns; layouts = NULL means every part is column-major, and the
 *                            handle is then left byte-identical to hades252_dmmcs_absorb with the same arguments.  All
 *                            parts of a call still run as ONE launch, whatever their layouts, shortest part first.  A part
 *                            with n_cols[p] = 0 is skipped whatever else it holds, its layout included.
 *   hades252_rmmcs_open_ex   hades252_dmmcs_open with a layout per committed matrix: d_rows and d_paths are what
 *                            hades252_dmmcs_open writes for the column-major twins.  An index >= h_0 gives an all-zero row
 *                            and an all-zero path: nothing outside the matrices and the tree is read.  Two launches: the
 *                            row gather -- one lane per (query, column) in output order, so for a row-major matrix
 *                            consecutive lanes read and write consecutive scalars -- and ONE call of
 *                            hades252_merkle_open_dev.
 * hades252_dmmcs_absorb and hades252_dmmcs_open are untouched and keep their own kernels; the _ex forms run one kernel
 * each that addresses a matrix through a row step and a column step the host computes from the layout.
 * Rules, all decided before the device is touched; a refused call allocates nothing and leaves the handle exactly as it
 * was.  The rules of hades252_dmmcs_absorb / hades252_dmmcs_open hold for the _ex forms (a NULL handle or array -- layouts
 * aside --, n_parts outside 1 .. 32, heights, alignment: device pointers are 16-byte aligned), and for a part that is not
 * skipped each of: a layout other than 0 or 1, a row-major strides[p] < n_cols[p] (column-major: strides[p] < n_rows[p]),
 * a byte count n_rows * stride * 32 (column-major: n_cols * stride * 32) that overflows size_t is
 * HADES252_ERR_INVALID_ARG.  absorb_rows: n_cols = 0 is a no-op success, even with NULL rows, and creates nothing; n_rows
 * outside 1 .. 2^30, NULL rows or rows that are not 8-byte aligned, row_stride < n_cols, a byte count that overflows
 * size_t, a column total that overflows uint64_t or a 33rd distinct height is HADES252_ERR_INVALID_ARG.  A HIP failure
 * inside a call returns HADES252_ERR_HIP and poisons the handle, as in f14 / f15.
 * No row-major form of f12 / f13 on their own (one group of a commitment is that stream), no witness form, no multiproofs. */
#define HADES252_LAYOUT_COLS 0   /* column-major: strides[p] is the plane stride (rows per plane) */
#define HADES252_LAYOUT_ROWS 1   /* row-major:    strides[p] is the row stride (scalars per row) */
int hades252_rmmcs_absorb_rows(void *mc, const uint64_t *rows, size_t n_rows, size_t n_cols, size_t row_stride);
int hades252_rmmcs_absorb_ex(void *mc, const void *const *d_mats, const uint64_t *n_rows, const uint64_t *n_cols,
                             const uint64_t *strides, const uint32_t *layouts, size_t n_parts, void *stream);
int hades252_rmmcs_open_ex(const void *mc, const void *const *d_mats, const uint64_t *n_rows, const uint64_t *n_cols,
                           const uint64_t *strides, const uint32_t *layouts, size_t n_parts,
                           const uint64_t *d_indices, size_t n_queries, void *d_rows, void *d_paths, void *stream);

/* ---- gadget witnesses of mixed-height commitment openings (f17): the fifth chain of row f4 ---- CONVENTION UNPINNED
 * What hades252_sponge_witness_dev and friends are for their chains, for an opening of a commitment of f14 / f15 / f16: the
 * chain a recursive verifier hashes most -- per query every group's row sponge, the injections and the path.  The family is
 * hades252_wmmcs_* ("w" for witness); the blocks of f14 to f16 stay true of their own calls.  Everything is in DEVICE
 * memory, on the caller's stream: the calls enqueue there and return; nothing is synchronised and nothing is downloaded.
 * The conventions are those of f14 (capacity, padding, the two tags: parameters, still unpinned), the shape arguments those
 * of hades252_dmmcs_verify with the same rules: heights and cols are HOST arrays, d_rows is query-major with the groups
 * concatenated tallest first, d_indices and d_paths as hades252_dmmcs_open writes them.  Scalars are four Montgomery limbs,
 * fully reduced and not checked, as everywhere.
 * One opening costs P = hades252_sponge_blocks(cols[g], pad_mode) summed over the groups + D + (G - 1) permutations, in the
 * order k_mmcs_verify walks them: group 0's blocks; the levels up to group 1's height; group 1's blocks; its injection; the
 * levels up to group 2's height; and so on up to the root.  A batch of n openings is P * n permutations, numbered
 * rec = t * n + q (step-major, query within the step, as in the sibling chain witnesses).  The state that enters step t of
 * query q:
 *   sponge, block 0 of a group's row   [capacity, v0, v1, v2, v3]: v_k is column k of the row; under pad_mode 1 a single 1
 *                                      sits in position cols[g]; zeros follow.
 *   sponge, block b > 0                the previous permutation's output with block b added into words 1..4 (the absorb add
 *                                      gates' outputs).
 *   inject                             [inject_tag, node, digest, 0, 0]: digest is word 1 of the previous permutation's output
 *                                      (the group's last block), node is word out_idx of the output of the last climb step
 *                                      before the group's sponge.
 *   climb                              [tag, the arity children, 0 ...]: the node sits at child position
 *                                      (index / arity^level) % arity with the level's arity - 1 siblings from d_paths around
 *                                      it, exactly as k_mmcs_verify places them.  The node is word out_idx of the last climb
 *                                      or inject output; for the first climb it is word 1 of group 0's last sponge output.
 * Indices are not range-checked, as in verify.  The gadget's selection, add and copy constraints (where the node sits, the
 * block added into words 1..4, the links between a record's input words and earlier records' outputs) are the consumer's: the
 * inputs carry their values, hades252_wmmcs_steps says which constraint belongs to which step.
 *   hades252_wmmcs_perms    P, or 0 for a shape hades252_mmcs_verify would refuse.  Pure host code.
 *   hades252_wmmcs_steps    the walk as data: steps[3 t ..] = (kind, group, ordinal) of step t, kind one of
 *                           HADES252_WMMCS_SPONGE / _INJECT / _CLIMB, ordinal the block number within the group's row, the
 *                           child level counted from the leaves (0 .. D - 1), or 0 for an injection; the group of a climb
 *                           step is the last group whose row has been hashed.  n_steps other than P is
 *                           HADES252_ERR_INVALID_ARG.  Pure host code, from the same closed-form count the launch uses.
 *   hades252_wmmcs_inputs   d_inputs receives P * n states of 160 B (the AoS format of the perm entry points) at rec * 160;
 *                           d_roots (may be NULL) receives n roots, byte for byte those of hades252_dmmcs_verify.  ONE launch
 *                           of k_mmcs_inputs: one query per lane, the walk of k_mmcs_verify with the five words stored in
 *                           front of every permutation.  Useful on its own: the inputs feed hades252_perm_witness_dev,
 *                           hades252_perm_trace_dev or hades252_perm_trace_scaled_dev, whichever form the circuit takes.
 *   hades252_wmmcs_witness  the inputs stage, then hades252_perm_witness_dev(d_inputs, d_wires, P * n, stream) on the same
 *                           stream: d_wires receives 972 * P * n scalars, wire-major.  Defining property, as for the sibling
 *                           chains: wires == hades252_perm_witness_dev(inputs) byte for byte, the P * n states taken as one
 *                           flat batch -- here by construction.  r2[out_idx] of the last step's record is the root.  NOT a
 *                           fused kernel: the chain is computed twice, once at the rate of the verification and once by the
 *                           witness kernel over independent records.  Measured (profiles/f17_mmcs_witness): 2^15 openings of
 *                           26 permutations take 1.80 x hades252_perm_witness_dev on the same records and 1.003 x the sum of
 *                           the two stages; the inputs stage of 2^18 openings takes 1.008 x hades252_dmmcs_verify.
 * Rules, all decided before the device is touched.  Those of hades252_dmmcs_verify (d_roots aside: it may be NULL, and is
 * 16-byte aligned if not); n_queries = 0 is a no-op success, even with NULL pointers; d_inputs must be non-NULL and 16-byte
 * aligned, and for the witness call d_wires too; P * n_queries above 2^30 is HADES252_ERR_INVALID_ARG; steps: a NULL or
 * misaligned steps, a refused shape.  A failed launch is HADES252_ERR_HIP with the thread's last HIP error set; there is no
 * handle to poison.
 * No one-opening-per-wave latency form, no fused kernel, no multiproofs. */
#define HADES252_WMMCS_SPONGE 0   /* a block of a group's row sponge */
#define HADES252_WMMCS_INJECT 1   /* the injection of a shorter group's row digest */
#define HADES252_WMMCS_CLIMB 2    /* a tree level */
size_t hades252_wmmcs_perms(const uint64_t *heights, const uint64_t *cols, size_t n_groups, int arity, int pad_mode);
int hades252_wmmcs_steps(const uint64_t *heights, const uint64_t *cols, size_t n_groups, int arity, int pad_mode,
                         uint32_t *steps, size_t n_steps);
int hades252_wmmcs_inputs(const void *d_rows, const uint64_t *heights, const uint64_t *cols, size_t n_groups,
                          const uint64_t *d_indices, const void *d_paths, size_t n_queries, int arity,
                          const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                          const uint64_t inject_tag_mont[4], int out_idx, void *d_inputs, void *d_roots, void *stream);
int hades252_wmmcs_witness(const void *d_rows, const uint64_t *heights, const uint64_t *cols, size_t n_groups,
                           const uint64_t *d_indices, const void *d_paths, size_t n_queries, int arity,
                           const uint64_t capacity_mont[4], int pad_mode, const uint64_t tag_mont[4],
                           const uint64_t inject_tag_mont[4], int out_idx, void *d_inputs, void *d_wires, void *d_roots,
                           void *stream);

/* ---- synthetic inputs and digests (benchmark / verification plumbing) --------------------- */
/* Generator B: scalar e (global element index first_elem + k) gets 4 splitmix64 limbs, top limb
 * masked to 62 bits (always < p); see DESIGN.md.  Stateless, so shards generate independently. */
int hades252_gen_b_dev(void *d_scalars, uint64_t first_elem, size_t n_elems, uint64_t seed, void *stream);
/* Generator A: scalar e has value first_elem + k (Montgomery form). */
int hades252_gen_a_dev(void *d_scalars, uint64_t first_elem, size_t n_elems, void *stream);
/* Position-sensitive 256-bit digest of n_u64 words: with g = first_index + i the global index
 * of word i, out[g % 4] += mix(word_i, g) (mod 2^64).  Additive over disjoint ranges, so
 * shards combine by limb-wise wrapping addition.  d_out4 = 4 device u64, zeroed by the call. */
int hades252_digest_dev(const void *d_words, uint64_t first_index, size_t n_u64, void *d_out4, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HADES252_H */
