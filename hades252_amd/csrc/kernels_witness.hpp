// kernels_witness.hpp -- gadget witnesses of permutation chains (extended): the sponge witness as one
// fused kernel, the input states of Merkle openings as a gather in front of k_perm_witness
// Part of the single translation unit hades252.hip (included there after kernels_perm.hpp); not a stand-alone header.
#pragma once

// A batch of n chains of S steps is S * n permutations, record rec = s * n + i (step-major, chain within the step): the
// lanes of a wave write consecutive records of every wire plane, as k_perm_witness does.  The record's input state goes to
// inputs[rec] (160 B, the AoS format of the perm entry points), its 972 gate outputs to the wire planes of length S * n --
// exactly what hades252_perm_witness_dev writes for those inputs.
//
// The two pieces below restate k_perm_witness (kernels_perm.hpp) operation for operation: the map of an in-memory state to
// the Rp form (witness_enter) and the round loop (witness_rounds).  Same helpers (store_wire, finalize32, mds_row_cols,
// mont_lin_words), same tables (d_wit), same fences and rolled loops, hence the same limbs and the same register budget.
// kernels_perm.hpp is left as it is because the committed counter records are keyed by its bytes; folding k_perm_witness
// onto these two is a follow-up for the next counter measurement.
constexpr int kWitnessLastRow = HADES_WITNESS_WIRES - 9;    // r2[0] of the last round; r2[j] is wire kWitnessLastRow + 2 j
__device__ __forceinline__ void witness_enter(const Fr (&in)[5], F29 (&y)[5]) {
#pragma unroll
    for (int w = 0; w < 5; w++) y[w] = to_f29(in[w]);
#pragma unroll 1
    for (int i = 0; i < 5; i++) {                       // in-memory limbs (x 2^256) -> x Rp
        int off = 0;                                    // opaque offset: the 81 multipliers stay inside the loop
        asm volatile("" : "+s"(off));
        y[4] = mont_lin(y[4], d_wit.in_lin + off);
        rotate_right(y);
#pragma unroll
        for (int w = 0; w < 5; w++)
#pragma unroll
            for (int k = 0; k < kNL; k++) limb_fence(y[w].l[k]);
    }
}

__device__ __forceinline__ void witness_rounds(F29 (&y)[5], uint8_t *__restrict__ wires, size_t plane, size_t rec, bool live) {
    int wire = 0;
#pragma unroll 1
    for (int r = 0; r < 67; r++) {
        const int32_t *c = d_wit.c[r], *ck = d_wit.ck[r];
        const bool full = r < 4 || r >= 63;
        if (r == 0) {
#pragma unroll 1
            for (int i = 0; i < 5; i++) {               // state after the first round key: word 4 - i sits at y[4]
                F29 s = y[4];
                add_lazy(s, c + (4 - i) * kNL);
                store_wire(wires, plane, wire + 4 - i, rec, live, finalize32(s));
                rotate_right(y);
            }
            wire += 5;
        }
        const int cnt = full ? 5 : 1;                   // S-boxes: every word (rotating through y[4]) or word 4 alone
#pragma unroll 1
        for (int i = 0; i < cnt; i++) {
            const int w = 4 - i;
            const int g = wire + (full ? 3 * w : 0);
            F29 z = y[4];
            add_lazy(z, c + w * kNL);
#pragma unroll
            for (int k = 0; k < kNL; k++) limb_fence(z.l[k]);
            F29 v2 = mont_sqr(z);
            store_wire(wires, plane, g, rec, live, finalize32(v2));
#pragma unroll
            for (int k = 0; k < kNL; k++) limb_fence(v2.l[k]);
            F29 v4 = mont_sqr(v2);
            store_wire(wires, plane, g + 1, rec, live, finalize32(v4));
#pragma unroll
            for (int k = 0; k < kNL; k++) {
                limb_fence(v4.l[k]);
                limb_fence(z.l[k]);
            }
            z = mont_mul(v4, z);
            store_wire(wires, plane, g + 2, rec, live, finalize32(z));
            y[4] = z;
            if (full) rotate_right(y);
#pragma unroll
            for (int w2 = 0; w2 < 5; w2++)
#pragma unroll
                for (int k = 0; k < kNL; k++) limb_fence(y[w2].l[k]);
        }
        wire += 3 * cnt;
        {                                               // U_w = Y_w lam 2^29 (+ the round constant of words 0..3, partial)
            int off = 0;
            asm volatile("" : "+s"(off));
            mont_lin_words<3>(y, d_wit.k_lin + off);
            int off2 = 0;
            asm volatile("" : "+s"(off2));
            mont_lin_words<2>(y + 3, d_wit.k_lin + off2);
            if (!full) {
#pragma unroll
                for (int w = 0; w < 4; w++) add_lazy(y[w], ck + w * kNL);
            }
        }
#pragma unroll 1
        for (int j = 0; j < 5; j++) {                   // r1[j]: columns 0..2 of row j
#pragma unroll
            for (int w = 0; w < 3; w++)
#pragma unroll
                for (int k = 0; k < kNL; k++) limb_fence(y[w].l[k]);
            store_wire(wires, plane, wire + 2 * j, rec, live, finalize32(mds_row_cols<3>(d_coop.mds[j], y)));
        }
        small_mds(y);
        const int32_t *cn = d_wit.c[r + 1];             // r2[j] = row j + the next round's constant (c[67] = 0)
#pragma unroll
        for (int j = 0; j < 5; j++) {
            F29 s = y[j];
            add_lazy(s, cn + j * kNL);
            store_wire(wires, plane, wire + 2 * j + 1, rec, live, finalize32(s));
        }
#pragma unroll
        for (int w = 0; w < 5; w++)
#pragma unroll
            for (int k = 0; k < kNL; k++) limb_fence(y[w].l[k]);
        wire += 10;
    }
}

// Sponge witness: lane i runs message i (the semantics of hades252_sponge_hash_dev: state = [capacity, 0, 0, 0, 0], block
// b of 4 scalars added to words 1..4, then a permutation; pad_mode 1 appends a single 1 first; at least one block) and
// records permutation b at rec = b * n + i.  Between blocks the state lives where the gadget has it: the last round's r2
// wires, in memory.  The lane reads its own five r2 records back (160 B against 31 104 B it has just written; its own
// earlier stores, so no fence) and adds the next block with fr_add, as the sponge kernels do: the state held across the
// chain costs no registers inside the round loop, which is why the budget is k_perm_witness's (three waves per SIMD, no
// scratch).  One message costs `blocks` x the latency of one k_perm_witness lane.  The digests (word 1 of the final states)
// are n consecutive records of one wire plane: the caller copies them out.
template <int PAD>
__global__ void __launch_bounds__(kBlock, 3) k_witness_sponge(const uint8_t *__restrict__ msgs, size_t n, size_t msg_len,
                                                              size_t blocks, Fr capacity, uint8_t *__restrict__ inputs,
                                                              uint8_t *__restrict__ wires) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    const size_t plane = blocks * n;
    // the state before block 0, [capacity, 0, 0, 0, 0], is parked in the lane's first input record (which block 0 then
    // overwrites): read back like every later state, the capacity holds no registers inside the chain.  (SGPR budget: the
    // chain carries as few uniform values as it can -- the step as the record offset `base`, the message as the words
    // still to come `rem` and a lane pointer, the padding as a template parameter.)
    if (live) {
        store_word(inputs + i * 160, capacity);
#pragma unroll
        for (int w = 1; w < 5; w++) store_word(inputs + i * 160 + w * 32, zero_word());
    }
    const uint8_t *mine = msgs + (live ? i * msg_len * 32 : 0);
    int64_t rem = (int64_t)msg_len;                     // message words from this block on (<= 4 * 2^30)
#pragma unroll 1
    for (size_t base = 0; base < plane; base += n) {    // base = b * n: step b
        const size_t rec = base + i;
        // the previous state: the parked one, or the previous permutation's output (r2 of its last round)
        const uint8_t *src = base == 0 ? inputs + i * 160 : wires + ((size_t)kWitnessLastRow * plane + rec - n) * 32;
        const size_t stride = base == 0 ? 32 : 2 * plane * 32;
        Fr in[5];
#pragma unroll
        for (int w = 0; w < 5; w++) in[w] = live ? load_word(src + w * stride) : zero_word();
#pragma unroll
        for (int k = 0; k < 4; k++) {                   // absorb: the gadget's add gates, words 1..4
            Fr v = live && k < rem ? load_word(mine + k * 32) : zero_word();
            if (PAD == 1 && k == rem) v = one_mont_word();
            in[1 + k] = fr_add(in[1 + k], v);
        }
        mine += 128;
        rem -= 4;
        if (live) {
#pragma unroll
            for (int w = 0; w < 5; w++) store_word(inputs + rec * 160 + w * 32, in[w]);
        }
        F29 y[5];
        witness_enter(in, y);
        witness_rounds(y, wires, plane, rec, live);
    }
}

// Merkle opening inputs: record rec = l * n_queries + q is the permutation that makes the level-(l + 1) ancestor of leaf
// indices[q]: [tag, the ARITY children of its group at level l (level 0 = the leaves, level l >= 1 = tree level l, the layout
// of hades252_merkle_build_dev), 0 ...]; a child position past the end of level l reads pad[l] (NULL: zero).  An index
// >= n_leaves reads nothing and gets all-zero states (counted once, at l = 0).  One thread per (record, word).
template <int ARITY>
__global__ void __launch_bounds__(kBlock) k_witness_path_states(const uint8_t *__restrict__ leaves,
                                                                const uint8_t *__restrict__ tree, size_t n_leaves, int depth,
                                                                const uint64_t *__restrict__ indices, size_t n_queries,
                                                                Fr tag, const uint8_t *__restrict__ pad,
                                                                uint8_t *__restrict__ inputs, int *bad_count) {
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t n_recs = (size_t)depth * n_queries;
    if (tid >= n_recs * 5) return;
    const size_t rec = tid / 5;
    const int w = (int)(tid - rec * 5);
    const int l = (int)(rec / n_queries);
    const size_t q = rec - (size_t)l * n_queries;
    size_t node = indices[q];
    Fr v = zero_word();
    if (node >= n_leaves) {
        if (l == 0 && w == 0 && bad_count != nullptr) atomicAdd(bad_count, 1);
    } else if (w == 0) {
        v = tag;
    } else if (w <= ARITY) {
        const uint8_t *level = leaves;
        size_t level_n = n_leaves, off = 0;
        for (int k = 0; k < l; k++) {
            node /= ARITY;
            level_n = (level_n + ARITY - 1) / ARITY;
            level = tree + off;
            off += level_n * 32;
        }
        const size_t child = node - node % ARITY + (size_t)(w - 1);
        if (child < level_n)
            v = load_word(level + child * 32);
        else
            v = load_pad(pad + (pad != nullptr ? (size_t)l * 32 : 0));
    }
    store_word(inputs + rec * 160 + (size_t)w * 32, v);
}

// Cipher witness (the construction of k_cipher, kernels_cipher.hpp; CONVENTION UNPINNED): lane i runs message i through
// S = ceil(M / 4) + 1 permutations, record rec = s * n + i.  inputs[0][i] = [D, M, kx, ky, nonce]; inputs[s][i] (s >= 1) =
// the output of permutation (s - 1, i) with words 1 + j absorbing word 4 (s - 1) + j of the message: encrypt adds it (the
// sums are the cipher words), decrypt replaces the state word by the cipher word reduced mod p (a 256-bit word is < 2.2 p:
// two conditional subtractions), so every input state is canonical, as perm_witness requires.  As in k_witness_sponge the
// state between steps is the last round's r2 wires in memory, read back by the lane that wrote them.
//   in   = messages (n x M, encrypt) or ciphers (n x (M + 1), decrypt)
//   out  = ciphers (n x (M + 1), encrypt) or messages (n x M, decrypt): what k_cipher writes; NULL: not written
//   ok_out, rejected (decrypt; each may be NULL): the verdict, as k_cipher gives it.  A rejected lane zeroes its message.
// SGPR budget: the round loop leaves k_witness_sponge's handful of SGPRs to the chain.  So the chain carries the step s
// (n, M and S * n are below 2^30: 32-bit), n, M and S, the decrypt lane's "every cipher word canonical" bit, and the
// pointers the rounds write (inputs, wires).  The four pointers of the absorb and the tail are parked in LDS and read back
// where they are used, behind an opaque index (so not hoisted into registers that live across the rounds).
struct CipherWitnessPtrs {
    const uint8_t *in;
    uint8_t *out, *ok_out;
    int *rejected;
};

__device__ __forceinline__ CipherWitnessPtrs cipher_witness_ptrs(const CipherWitnessPtrs *parked) {
    int z = 0;
    asm volatile("" : "+s"(z));
    return parked[z];
}

template <bool DECRYPT>
__global__ void __launch_bounds__(kBlock, 3) k_witness_cipher(const uint8_t *__restrict__ in, const uint8_t *__restrict__ keys,
                                                              const uint8_t *__restrict__ nonces, uint32_t n, uint32_t len,
                                                              uint32_t steps, Fr domain, Fr len_word,
                                                              uint8_t *__restrict__ inputs, uint8_t *__restrict__ wires,
                                                              uint8_t *__restrict__ out, uint8_t *__restrict__ ok_out,
                                                              int *rejected) {
    __shared__ CipherWitnessPtrs parked[1];
    if (threadIdx.x == 0) parked[0] = CipherWitnessPtrs{in, out, ok_out, rejected};
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    const uint32_t plane = steps * n;
    const uint32_t in_stride = DECRYPT ? len + 1 : len, out_stride = DECRYPT ? len : len + 1;
    // step 0's state, parked in the lane's first input record and read back like every later state (the domain, length,
    // key and nonce hold no registers inside the chain)
    if (live) {
        store_word(inputs + i * 160, domain);
        store_word(inputs + i * 160 + 32, len_word);
        store_word(inputs + i * 160 + 64, load_word(keys + i * 64));
        store_word(inputs + i * 160 + 96, load_word(keys + i * 64 + 32));
        store_word(inputs + i * 160 + 128, load_word(nonces + i * 32));
    }
    bool good = true;                                   // decrypt: every cipher word so far canonical
#pragma unroll 1
    for (uint32_t s = 0; s < steps; s++) {
        const size_t rec = (size_t)s * n + i;
        const uint8_t *src = s == 0 ? inputs + i * 160 : wires + ((size_t)kWitnessLastRow * plane + rec - n) * 32;
        const size_t stride = s == 0 ? 32 : (size_t)2 * plane * 32;
        Fr st[5];
#pragma unroll
        for (int w = 0; w < 5; w++) st[w] = live ? load_word(src + w * stride) : zero_word();
        if (s != 0) {                                   // absorb words 4 (s - 1) + j (those < M): the gadget's add gates
            const CipherWitnessPtrs p = cipher_witness_ptrs(parked);
            const uint32_t w0 = 4 * (s - 1);
            const uint8_t *src_w = p.in + (live ? (i * in_stride + w0) * 32 : 0);
            uint8_t *dst_w = p.out + (live && p.out != nullptr ? (i * out_stride + w0) * 32 : 0);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (w0 + j < len) {
                    const Fr c = live ? load_word(src_w + j * 32) : zero_word();
                    Fr o;
                    if constexpr (DECRYPT) {
                        good = good && fr_is_canonical(c);
                        const Fr cr = fr_cond_sub_p(fr_cond_sub_p(c));
                        o = fr_sub(cr, st[1 + j]);
                        st[1 + j] = cr;
                    } else {
                        st[1 + j] = fr_add(st[1 + j], c);
                        o = st[1 + j];
                    }
                    if (live && p.out != nullptr) store_word(dst_w + j * 32, o);
                }
            }
        }
        if (live) {
#pragma unroll
            for (int w = 0; w < 5; w++) store_word(inputs + rec * 160 + w * 32, st[w]);
        }
        F29 y[5];
        witness_enter(st, y);
        witness_rounds(y, wires, plane, rec, live);
    }
    // the tag: word 1 of the final state, r2[1] of the last round of the lane's last record
    const CipherWitnessPtrs p = cipher_witness_ptrs(parked);
    const size_t last = (size_t)(plane - n) + i;
    const Fr tag = live ? load_word(wires + ((size_t)(kWitnessLastRow + 2) * plane + last) * 32) : zero_word();
    if constexpr (!DECRYPT) {
        if (live && p.out != nullptr) store_word(p.out + (i * out_stride + len) * 32, tag);
    } else {
        const Fr c = live ? load_word(p.in + (i * in_stride + len) * 32) : zero_word();
        good = good && fr_is_canonical(c) && fr_eq(c, tag);
        if (live && !good && p.out != nullptr) {        // a rejected message comes out as M zero words, as from k_cipher
#pragma unroll 1
            for (uint32_t k = 0; k < len; k++) store_word(p.out + (i * out_stride + k) * 32, zero_word());
        }
        if (live && p.ok_out != nullptr) p.ok_out[i] = good ? 1 : 0;
        const uint64_t rej = __ballot(live && !good);
        if ((threadIdx.x & (kWave - 1)) == 0 && rej != 0 && p.rejected != nullptr) atomicAdd(p.rejected, (int)__popcll(rej));
    }
}

// Duplex sponge witness (the construction of k_safe, kernels_safe.hpp; CONVENTION UNPINNED): lane i runs sponge i through
// the n_perms permutations the host counted for the calls (abi_safe.hpp), the t-th of them record rec = (step0 + t) * n + i
// of planes of length total * n.  Between two permutations a sponge emits j words and then adds k words (one SafeStep of
// the unchanged, wave-uniform walk): the emitted words are read from the state just loaded (to out, per lane, when out is
// there), the added ones go in with fr_add from a per-lane load_word, as k_witness_sponge reads its blocks -- the traffic
// is ~1 % of a record's 31 KB of wires, so no LDS slab.  As in the sibling chains the state between permutations is the
// last round's r2 wires in memory, read back by the lane that wrote them; the state of the call's first step is read from
// `states` (streaming) or, states == NULL (one-shot: a fresh sponge that ends with the launch), from the lane's first input
// record, where [tag, 0, 0, 0, 0] is parked first.  After the last permutation the loop body runs once more: the final
// step (the last emits; in streaming also trailing adds), and the five state words go to `states` instead of an input
// record -- ONE store site with a selected destination, so that nothing but the round loop consumes st[] after the step.
// A call without a permutation (streaming, n_perms = 0) writes no record at all.
// SGPR budget: the round loop leaves a chain a handful of SGPRs.  The chain carries the step t, n, n_perms, step0, total
// and the two pointers the rounds write.  Everything the step alone needs is parked in LDS and read back at the top of
// every step behind an opaque index: the constants of the launch once per block, the walk and the two word offsets in a
// slot per wave (waves of a block do not run in lockstep: no block barrier belongs inside the loop).  The parked values
// are uniform: every lane of a wave stores the same value and reads back only what it wrote itself, so no cross-lane
// ordering arises; they are left as the per-lane values the LDS read returns.  The 64 call words are copied to LDS once
// (static indices, one thread, the barrier before the loop) and indexed there: a dynamically indexed 256-byte by-value
// argument costs the round loop its registers.  No one-per-wave latency form, as for the other chain witnesses.
struct DuplexWitnessConst {
    const uint8_t *in;
    uint8_t *out, *states;
    uint32_t n_in, n_out, n_calls, pad;
};
struct DuplexWitnessSlot {
    SafeWalk walk;
    uint32_t in_off, out_off;
};

__global__ void __launch_bounds__(kBlock, 3) k_witness_duplex(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                              uint8_t *states, uint32_t n, uint32_t n_in, uint32_t n_out,
                                                              SafeCalls calls, uint32_t n_calls, uint32_t cursor,
                                                              uint32_t n_perms, uint32_t step0, uint32_t total, Fr tag,
                                                              uint8_t *__restrict__ inputs, uint8_t *__restrict__ wires) {
    __shared__ SafeCalls parked_calls;
    __shared__ DuplexWitnessConst parked_const[1];
    __shared__ DuplexWitnessSlot parked_slot[kWavesPerBlock];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < HADES252_SAFE_MAX_CALLS; c++) parked_calls.c[c] = calls.c[c];
        parked_const[0] = DuplexWitnessConst{in, out, states, n_in, n_out, n_calls, 0};
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    const int wave = threadIdx.x / kWave;
    {
        DuplexWitnessSlot first;
        first.walk = safe_begin(parked_calls, cursor);
        first.in_off = first.out_off = 0;
        parked_slot[wave] = first;
    }
    if (states == nullptr && live) {                    // one-shot: n_perms >= 1, so the record exists
        uint8_t *park = inputs + ((size_t)step0 * n + i) * 160;
        store_word(park, tag);
#pragma unroll
        for (int w = 1; w < 5; w++) store_word(park + w * 32, zero_word());
    }
#pragma unroll 1
    for (uint32_t t = 0;; t++) {
        int z = 0;
        asm volatile("" : "+s"(z));
        const DuplexWitnessConst k = parked_const[z];
        DuplexWitnessSlot slot = parked_slot[wave + z];
        const size_t plane = (size_t)total * n;
        const size_t rec = (size_t)(step0 + t) * n + i;
        // the previous state: the caller's or the parked one, or the previous permutation's output (r2 of its last round)
        const uint8_t *src = t != 0             ? wires + ((size_t)kWitnessLastRow * plane + rec - n) * 32
                             : k.states != nullptr ? k.states + (size_t)i * 160
                                                   : inputs + rec * 160;
        const size_t stride = t != 0 ? 2 * plane * 32 : 32;
        Fr st[5];
#pragma unroll
        for (int w = 0; w < 5; w++) st[w] = live ? load_word(src + w * stride) : zero_word();
        const SafeStep s = safe_step(parked_calls, k.n_calls, slot.walk);
        if (s.j > 0 && live && k.out != nullptr) {      // emit: read, not changed
            uint8_t *dst = k.out + ((size_t)i * k.n_out + slot.out_off) * 32;
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (p >= s.e0 && p < s.e0 + s.j) store_word(dst + (p - s.e0) * 32, st[1 + p]);
        }
        if (s.k > 0) {                                  // absorb: the gadget's add gates
            const uint8_t *from = k.in + (live ? ((size_t)i * k.n_in + slot.in_off) * 32 : 0);
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (p >= s.a0 && p < s.a0 + s.k)
                    st[1 + p] = fr_add(st[1 + p], live ? load_word(from + (p - s.a0) * 32) : zero_word());
        }
        slot.out_off += s.j;
        slot.in_off += s.k;
        safe_permuted(parked_calls, k.n_calls, slot.walk);     // (after the last permutation the walk is not read again)
        parked_slot[wave + z] = slot;
        const bool last = t == n_perms;
        if (live && !(last && k.states == nullptr)) {       // (no pointer is formed from a NULL k.states)
            uint8_t *dst = last ? k.states + (size_t)i * 160 : inputs + rec * 160;
#pragma unroll
            for (int w = 0; w < 5; w++) store_word(dst + w * 32, st[w]);
        }
        if (last) break;
        F29 y[5];
        witness_enter(st, y);
        witness_rounds(y, wires, plane, rec, live);
    }
}
