// kernels_wmmcs.hpp -- gadget witnesses of mixed-height commitment openings: the input state of every permutation of the chain
// k_mmcs_verify walks (kernels_mmcs.hpp), written out for hades252_perm_witness_dev and friends (abi_wmmcs.hpp).
// Part of the single translation unit hades252.hip (included there after kernels_rowmajor.hpp); not a stand-alone header.
#pragma once

// Lane q walks the chain of opening q exactly as k_mmcs_verify does -- the same arguments, the same phases, the same single
// fast_perm call site in one loop, the group table MmcsGroups and the step kinds kMmcs* of kernels_mmcs.hpp -- and, in front of
// every permutation, stores the five words that enter it: step t of query q is record rec = t * n + q (step-major, query
// within the step, as in the sibling chain witnesses), 160 B in the AoS format of the perm entry points at inputs + rec * 160.
// Consecutive lanes own consecutive records of a step: 10 KiB contiguous over the wave per step.  roots may be NULL; else
// roots[q] is what k_mmcs_verify stores.  No LDS, no barrier, no scratch: registers alone decide the residency
// (__launch_bounds__(256, 3): at most 168 VGPRs).  Every branch depends on kernel arguments only and is wave-uniform, but for
// the choice of a sibling's slot.  A lane past the last query leaves at once: it reads and writes nothing.
template <int ARITY>
__global__ void __launch_bounds__(kBlock, 3) k_mmcs_inputs(const uint8_t *__restrict__ rows, const uint64_t *__restrict__ indices,
                                                           const uint8_t *__restrict__ paths, size_t n, MmcsGroups groups,
                                                           uint32_t n_groups, size_t row_cols, uint32_t depth, size_t n_perms,
                                                           int pad_mode, Fr capacity, Fr tag, Fr inject_tag, int out_idx,
                                                           uint8_t *__restrict__ inputs, uint8_t *__restrict__ roots) {
    const size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const uint8_t *row = rows + q * row_cols * 32;                     // the open group's row; moves on group by group
    const uint8_t *sib = paths + q * (size_t)depth * (ARITY - 1) * 32;  // the next level's siblings; moves on level by level
    uint64_t idx = indices[q];
    Fr st[5], node = zero_word();
#pragma unroll
    for (int w = 0; w < 5; w++) st[w] = zero_word();
    uint32_t g = 0, phase = kMmcsSponge, c = 0;                        // c: columns of the open row taken so far
    uint32_t cols = groups.cols[0];
    uint32_t left = (cols + (pad_mode == 1 ? 1u : 0u) + 3) / 4;        // blocks, or levels, before the phase ends
#pragma unroll 1
    for (size_t t = 0; t < n_perms; t++) {
        if (phase == kMmcsSponge) {
            if (c == 0) {
                st[0] = capacity;
#pragma unroll
                for (int w = 1; w < 5; w++) st[w] = zero_word();
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t at = c + (uint32_t)k;
                Fr v;
                if (at < cols)
                    v = load_word(row + (size_t)at * 32);
                else
                    v = fr_select(pad_mode == 1 && at == cols, one_mont_word(), zero_word());
                st[1 + k] = fr_add(st[1 + k], v);
            }
            c += 4;
        } else if (phase == kMmcsInject) {
            st[0] = inject_tag;
            st[2] = st[1];                                             // the digest the sponge just left in word 1
            st[1] = node;                                              // it waited for this digest in its registers
            st[3] = zero_word();
            st[4] = zero_word();
        } else {
            const int pos = (int)(idx % ARITY);
            idx /= ARITY;
            st[0] = tag;
#pragma unroll
            for (int w = 1; w < 5; w++) st[w] = zero_word();
#pragma unroll
            for (int ch = 0; ch < ARITY; ch++) {                       // child ch: the node itself at `pos`, else the next sibling
                Fr v = node;
                if (ch != pos) v = load_word(sib + (size_t)(ch < pos ? ch : ch - 1) * 32);
                st[1 + ch] = v;
            }
            sib += (ARITY - 1) * 32;
        }
#pragma unroll
        for (int w = 0; w < 5; w++) store_word(inputs + (t * n + q) * 160 + w * 32, st[w]);   // what enters permutation (t, q)
        Fr out[5];
        fast_perm<5>(&d_fast, st, out, 0);
#pragma unroll
        for (int w = 0; w < 5; w++) st[w] = out[w];
        if (phase == kMmcsSponge) {
            if (--left == 0) {                                         // the row's digest is st[1]
                row += (size_t)cols * 32;
                if (g == 0) {
                    node = st[1];
                    phase = kMmcsClimb;
                    left = groups.climb[0];
                } else {
                    phase = kMmcsInject;
                }
            }
        } else {
#pragma unroll
            for (int w = 0; w < 5; w++)
                if (w == out_idx) node = st[w];
            if (phase == kMmcsInject) {
                phase = kMmcsClimb;
                left = groups.climb[g];
            } else {
                left--;
            }
            if (left == 0 && g + 1 < n_groups) {                       // the next group's height is reached: its row, then inject
                g++;
                phase = kMmcsSponge;
                c = 0;
                cols = groups.cols[g];
                left = (cols + (pad_mode == 1 ? 1u : 0u) + 3) / 4;
            }
        }
    }
    if (roots != nullptr) store_word(roots + q * 32, node);
}
