// kernels_mmcs.hpp -- mixed-height matrix commitments: the injection of a shorter matrix's row digests into a tree level, and
// the verification of a whole opening (every group's row, the injections, the path) in one launch (host_mmcs.hpp).
// Part of the single translation unit hades252.hip (included there after kernels_matrix_stream.hpp); not a stand-alone header.
#pragma once

// Both kernels: one item per lane, consecutive lanes own consecutive items, every word is a per-lane load_word / store_word
// (32 contiguous bytes per lane, 2 KiB contiguous over the wave where the items are digests).  No LDS, no barrier, no
// scratch: registers alone decide the residency (__launch_bounds__(256, 3): at most 168 VGPRs).  Every branch depends on
// kernel arguments only and is wave-uniform, but for the choice of a sibling's slot, which is k_merkle_verify's; the state
// words are indexed by unrolled constants.  A lane past the last item leaves at once: it reads and writes nothing.

// nodes[i] = perm([inject_tag, nodes[i], leaf[i], 0, 0])[out_idx] for i < n, in place: the parent hades252_merkle_level_dev
// gives at arity 2 for the pair (nodes[i], leaf[i]) under the tag inject_tag.
__global__ void __launch_bounds__(kBlock, 3) k_mmcs_inject(uint8_t *__restrict__ nodes, const uint8_t *__restrict__ leaf, size_t n,
                                                           Fr inject_tag, int out_idx) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Fr st[5];
    st[0] = inject_tag;
    st[1] = load_word(nodes + i * 32);
    st[2] = load_word(leaf + i * 32);
    st[3] = zero_word();
    st[4] = zero_word();
    Fr out[1];
    fast_perm<1>(&d_fast, st, out, out_idx);
    store_word(nodes + i * 32, out[0]);
}

// The shape of a commitment as the verifier walks it, tallest group first: the columns of group g and the tree levels
// between its height and the next group's (the last group's: up to the root).  By value in the kernel arguments.
struct MmcsGroups {
    uint32_t cols[HADES252_MMCS_MAX_GROUPS];
    uint32_t climb[HADES252_MMCS_MAX_GROUPS];
};

enum { kMmcsSponge = 0, kMmcsInject = 1, kMmcsClimb = 2 };

// Lane q recomputes the root from opening q.  rows: n x row_cols scalars, query-major, the opened rows of all groups
// concatenated (tallest first); paths: n x depth x (ARITY - 1) siblings in the layout of hades252_merkle_open_dev.
// The chain of lane q, n_perms = sum of the groups' sponge blocks + depth + (n_groups - 1) permutations (the host counts
// them in closed form), all through ONE fast_perm call site in one loop, as k_safe does:
//   sponge   the blocks of group g's row: the state starts as [capacity, 0, 0, 0, 0], every block of four columns is added
//            into words 1..4 and permuted; the pad scalar as planes_word places it; the digest is word 1;
//   inject   (g > 0) [inject_tag, node, digest, 0, 0] -> node: the node waited for this digest parked in its registers;
//   climb    climb[g] levels: [tag, children, 0 ..] -> node, the node at position index % ARITY and the level's siblings
//            around it, as in k_merkle_verify; then the next group's sponge.
// What a step is follows from the group table and the counts alone, so the walk is scalar work.
template <int ARITY>
__global__ void __launch_bounds__(kBlock, 3) k_mmcs_verify(const uint8_t *__restrict__ rows, const uint64_t *__restrict__ indices,
                                                           const uint8_t *__restrict__ paths, size_t n, MmcsGroups groups,
                                                           uint32_t n_groups, size_t row_cols, uint32_t depth, size_t n_perms,
                                                           int pad_mode, Fr capacity, Fr tag, Fr inject_tag, int out_idx,
                                                           uint8_t *__restrict__ roots) {
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
    store_word(roots + q * 32, node);
}
