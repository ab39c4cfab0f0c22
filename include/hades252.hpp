// hades252.hpp -- C++ host-side mirror of the reference's operator interface, over the C ABI.
//
// The reference is compiled code (Rust) and this image has no Rust toolchain, so the host side
// above the C ABI is written in C++.  Names, argument meaning and failure behaviour follow
//   pub trait Strategy<T>           reference src/strategies.rs:31-163
//   pub struct ScalarStrategy       reference src/strategies/scalar.rs:11-50
//   WIDTH / TOTAL_FULL_ROUNDS / PARTIAL_ROUNDS   reference src/lib.rs:20-27
// batched: where the reference takes `&mut [BlsScalar]` of exactly WIDTH words, these methods take
// any whole number of WIDTH-word states and apply the operation to each, in place.
// Header-only; link with -lhades252 (and the HIP runtime for device buffers).
//
// Size switch: the Rust binding (rust/src/hip.rs, MIN_GPU_STATES = 2) sends a call that carries ONE state to the
// reference's own CPU `ScalarStrategy` (one GPU call costs ~65 us, one CPU permutation ~50 us).  This mirror has NO
// CPU path, on purpose -- there is no reference CPU code in a C++ caller's crate to delegate to, and a CPU leg inside
// this library would be an oracle in the product: every call here goes to the device or throws.
#ifndef HADES252_HPP
#define HADES252_HPP

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "hades252.h"

namespace dusk_hades {

constexpr std::size_t WIDTH = HADES252_WIDTH;                          // src/lib.rs:27
constexpr std::size_t TOTAL_FULL_ROUNDS = HADES252_TOTAL_FULL_ROUNDS;  // src/lib.rs:21
constexpr std::size_t PARTIAL_ROUNDS = HADES252_PARTIAL_ROUNDS;        // src/lib.rs:25

// In-memory BlsScalar of dusk-bls12_381: 4 x u64 little-endian Montgomery limbs.
struct BlsScalar {
    std::uint64_t limbs[4];
};
static_assert(sizeof(BlsScalar) == 32, "BlsScalar must be 32 bytes");

// The reference panics (and aborts: Cargo.toml:20); the mirror throws.
struct HadesPanic : std::runtime_error {
    int code;
    HadesPanic(const std::string &what, int c) : std::runtime_error(what), code(c) {}
};

inline void check(int rc, const char *where) {
    if (rc != HADES252_OK)
        throw HadesPanic(std::string(where) + ": " + hades252_strerror(rc), rc);
}

// `ROUND_CONSTANTS.iter()` (src/strategies.rs:141): a cursor into the device-resident table.
struct RoundConstantsIter {
    std::size_t pos = 0;
    static constexpr std::size_t CONSTANTS = 960;          // src/round_constants.rs:18
};

// A device-resident batch of states (caller-owned memory on the current HIP device).
struct DeviceStates {
    void *ptr;
    std::size_t n_states;
    void *stream;   // hipStream_t, nullptr = default stream
};

template <typename T>
class Strategy {
public:
    virtual ~Strategy() = default;

    // src/strategies.rs:33-41
    static std::size_t next_c(RoundConstantsIter &constants) {
        if (constants.pos >= RoundConstantsIter::CONSTANTS) throw HadesPanic("Hades252 out of ARK constants", -1);
        return constants.pos++;
    }
    virtual void add_round_key(RoundConstantsIter &constants, T words) = 0;   // src/strategies.rs:50-52
    virtual void quintic_s_box(T value) = 0;                                  // src/strategies.rs:59
    virtual void mul_matrix(RoundConstantsIter &constants, T values) = 0;     // src/strategies.rs:63-65
    virtual void apply_partial_round(RoundConstantsIter &constants, T words) = 0;   // :79-93
    virtual void apply_full_round(RoundConstantsIter &constants, T words) = 0;      // :107-119
    virtual void perm(T data) = 0;                                                  // :140-157
    static std::size_t rounds() { return TOTAL_FULL_ROUNDS + PARTIAL_ROUNDS; }      // :160-162
};

// GPU-backed ScalarStrategy.  Stateless like the reference's zero-sized struct.
class ScalarStrategy : public Strategy<DeviceStates> {
    // any cursor is legal (src/strategies.rs:33-41); past the 960 constants the reference panics
    static int cursor_of(RoundConstantsIter &c) {
        if (c.pos + WIDTH > RoundConstantsIter::CONSTANTS) throw HadesPanic("Hades252 out of ARK constants", -6);
        return static_cast<int>(c.pos);
    }
    static void advance(RoundConstantsIter &c) {
        for (std::size_t i = 0; i < WIDTH; i++) next_c(c);
    }

public:
    static ScalarStrategy new_() { return ScalarStrategy(); }   // src/strategies/scalar.rs:17-19

    void add_round_key(RoundConstantsIter &constants, DeviceStates w) override {   // scalar.rs:23-30
        check(hades252_add_round_key_at_dev(w.ptr, w.n_states, cursor_of(constants), w.stream),
              "add_round_key");
        advance(constants);
    }
    // every 32-byte scalar of the batch (n_states counts scalars here)
    void quintic_s_box(DeviceStates v) override {                                   // scalar.rs:32-34
        check(hades252_quintic_s_box_dev(v.ptr, v.n_states, v.stream), "quintic_s_box");
    }
    void mul_matrix(RoundConstantsIter &, DeviceStates v) override {                // scalar.rs:36-49
        check(hades252_mul_matrix_dev(v.ptr, v.n_states, v.stream), "mul_matrix");
    }
    void apply_partial_round(RoundConstantsIter &constants, DeviceStates w) override {
        check(hades252_apply_partial_round_at_dev(w.ptr, w.n_states, cursor_of(constants), w.stream),
              "apply_partial_round");
        advance(constants);
    }
    void apply_full_round(RoundConstantsIter &constants, DeviceStates w) override {
        check(hades252_apply_full_round_at_dev(w.ptr, w.n_states, cursor_of(constants), w.stream),
              "apply_full_round");
        advance(constants);
    }
    void perm(DeviceStates data) override {
        check(hades252_perm_batch_dev(data.ptr, data.n_states, data.stream), "perm");
    }

    // `strategy.perm(&mut state)` on host memory: len must be a multiple of WIDTH
    // (the reference panics for len != WIDTH, scalar.rs:48).
    void perm(BlsScalar *data, std::size_t len) {
        if (len % WIDTH != 0) throw HadesPanic("perm: slice length is not a multiple of WIDTH", -1);
        check(hades252_perm_batch(reinterpret_cast<std::uint64_t *>(data), len / WIDTH), "perm");
    }
};

// A batch of states in page-locked host memory (hades252_host_alloc): `perm` on it goes straight to DMA instead of
// page-locking the slice inside every call.  Movable, frees on destruction.
class PinnedStates {
    BlsScalar *p_ = nullptr;
    std::size_t len_ = 0;

public:
    explicit PinnedStates(std::size_t n_states) : len_(n_states * WIDTH) {
        void *raw = nullptr;
        check(hades252_host_alloc(&raw, (len_ ? len_ : 1) * sizeof(BlsScalar)), "host_alloc");
        p_ = static_cast<BlsScalar *>(raw);
    }
    PinnedStates(const PinnedStates &) = delete;
    PinnedStates &operator=(const PinnedStates &) = delete;
    PinnedStates(PinnedStates &&o) noexcept : p_(o.p_), len_(o.len_) { o.p_ = nullptr; o.len_ = 0; }
    ~PinnedStates() { if (p_) (void)hades252_host_free(p_); }
    BlsScalar *data() { return p_; }
    std::size_t len() const { return len_; }          // scalars: WIDTH per state
};

// Device memory through the library alone (hades252_dev_alloc / _upload / _download): a caller that does not link HIP
// keeps its data resident and feeds the `DeviceStates` of the strategy above.  Movable, frees on destruction.
class DeviceBuffer {
    void *p_ = nullptr;
    std::size_t bytes_ = 0;

public:
    explicit DeviceBuffer(std::size_t bytes) : bytes_(bytes) { check(hades252_dev_alloc(&p_, bytes ? bytes : 16), "dev_alloc"); }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    ~DeviceBuffer() { if (p_) (void)hades252_dev_free(p_); }
    void *ptr() const { return p_; }
    std::size_t bytes() const { return bytes_; }
    void upload(const void *host, std::size_t bytes, void *stream = nullptr) { check(hades252_dev_upload(p_, host, bytes, stream), "dev_upload"); }
    void download(void *host, std::size_t bytes, void *stream = nullptr) const {
        check(hades252_dev_download(host, p_, bytes, stream), "dev_download");
        check(hades252_stream_sync(stream), "stream_sync");
    }
};

// The callers of `perm` on host memory (dusk-poseidon's node and sponge shapes, README.md:9; tag / out_idx / capacity /
// padding are that crate's convention and parameters here).
inline BlsScalar merkle_root(const BlsScalar *leaves, std::size_t n_leaves, int arity, const BlsScalar &tag, int out_idx = 1,
                             const BlsScalar *pad = nullptr) {
    BlsScalar root{};
    check(hades252_merkle_root(reinterpret_cast<const std::uint64_t *>(leaves), n_leaves, arity, tag.limbs, out_idx,
                               reinterpret_cast<const std::uint64_t *>(pad), root.limbs), "merkle_root");
    return root;
}

inline void sponge_hash(const BlsScalar *msgs, std::size_t n_msgs, std::size_t msg_len, const BlsScalar &capacity, bool pad_one,
                        BlsScalar *digests) {
    check(hades252_sponge_hash(reinterpret_cast<const std::uint64_t *>(msgs), n_msgs, msg_len, capacity.limbs, pad_one ? 1 : 0,
                               reinterpret_cast<std::uint64_t *>(digests)), "sponge_hash");
}

// The batched Poseidon cipher on host memory (dusk-poseidon's PoseidonCipher shape; CONVENTION UNPINNED, include/hades252.h).
// msgs: n x msg_len, keys: n x 2, nonces: n, ciphers: n x (msg_len + 1) scalars.  The crate's domain word is 2^32:
// CIPHER_DOMAIN.
constexpr BlsScalar CIPHER_DOMAIN{HADES252_CIPHER_DOMAIN_MONT};
inline void cipher_encrypt(const BlsScalar *msgs, const BlsScalar *keys, const BlsScalar *nonces, std::size_t n_msgs,
                           std::size_t msg_len, const BlsScalar &domain, BlsScalar *ciphers) {
    check(hades252_cipher_encrypt(reinterpret_cast<const std::uint64_t *>(msgs), reinterpret_cast<const std::uint64_t *>(keys),
                                  reinterpret_cast<const std::uint64_t *>(nonces), n_msgs, msg_len, domain.limbs,
                                  reinterpret_cast<std::uint64_t *>(ciphers)),
          "cipher_encrypt");
}

// ok[i] = 1 if cipher i authenticated (its message words in msgs), 0 if not (its message words zero); returns the number
// of rejected messages.
inline std::size_t cipher_decrypt(const BlsScalar *ciphers, const BlsScalar *keys, const BlsScalar *nonces, std::size_t n_msgs,
                                  std::size_t msg_len, const BlsScalar &domain, BlsScalar *msgs, std::uint8_t *ok) {
    std::size_t rejected = 0;
    check(hades252_cipher_decrypt(reinterpret_cast<const std::uint64_t *>(ciphers), reinterpret_cast<const std::uint64_t *>(keys),
                                  reinterpret_cast<const std::uint64_t *>(nonces), n_msgs, msg_len, domain.limbs,
                                  reinterpret_cast<std::uint64_t *>(msgs), ok, &rejected),
          "cipher_decrypt");
    return rejected;
}

// The batched duplex sponge (dusk-safe's SAFE sponge; CONVENTION UNPINNED, include/hades252.h).  A call of an IO pattern is
// one word: safe_absorb(n) / safe_squeeze(n).
constexpr std::uint32_t safe_absorb(std::uint32_t n) { return HADES252_SAFE_ABSORB | n; }
constexpr std::uint32_t safe_squeeze(std::uint32_t n) { return n; }
struct SafePattern {
    std::size_t n_in, n_out, n_perms;      // words absorbed / squeezed and permutations, per sponge
};
// Validates a pattern (no device needed); panics on an invalid one.
inline SafePattern safe_pattern(const std::uint32_t *calls, std::size_t n_calls) {
    SafePattern p{0, 0, 0};
    check(hades252_safe_pattern(calls, n_calls, &p.n_in, &p.n_out, &p.n_perms), "safe_pattern");
    return p;
}
// Host memory: in n_msgs x n_in, out n_msgs x n_out scalars, message-major.
inline void safe_hash(const BlsScalar *in, std::size_t n_msgs, const std::uint32_t *calls, std::size_t n_calls,
                      const BlsScalar &tag, BlsScalar *out) {
    check(hades252_safe_hash(reinterpret_cast<const std::uint64_t *>(in), n_msgs, calls, n_calls, tag.limbs,
                             reinterpret_cast<std::uint64_t *>(out)), "safe_hash");
}
// Proof-of-work grinding, host memory (include/hades252.h, CONVENTION UNPINNED: tests/grind_model.py): per job (a seed of five
// scalars) the smallest nonce x in [first_nonce, first_nonce + max_nonces) for which word out_idx of perm(seed with
// seed[word] + x) is, as a canonical integer, strictly below `target` (4 limbs, little-endian, NOT Montgomery).
// found[j] = 1 and nonces[j] = the nonce, or found[j] = 0 and nonces[j] untouched.
inline void grind(const BlsScalar *seeds, std::size_t n_jobs, int word, int out_idx, const std::uint64_t target[4],
                  std::uint64_t first_nonce, std::uint64_t max_nonces, std::uint64_t *nonces, std::uint8_t *found) {
    check(hades252_grind(reinterpret_cast<const std::uint64_t *>(seeds), n_jobs, word, out_idx, target, first_nonce, max_nonces,
                         nonces, found), "grind");
}
// The permutation run backwards, host memory, in place (include/hades252.h): perm(perm_inverse(y)) == y.  perm_inverse_rounds
// undoes rounds round_hi - 1, ..., round_lo only (the state after round round_hi - 1 in, the state after round round_lo - 1
// out; 0 <= round_lo <= round_hi <= HADES252_ROUNDS_TOTAL); fifth_root is x -> x^(1/5) on independent scalars.
inline void perm_inverse(BlsScalar *states, std::size_t n_perms) {
    check(hades252_perm_inverse_batch(reinterpret_cast<std::uint64_t *>(states), n_perms), "perm_inverse");
}
inline void perm_inverse_rounds(BlsScalar *states, std::size_t n_perms, int round_hi, int round_lo) {
    check(hades252_perm_inverse_rounds(reinterpret_cast<std::uint64_t *>(states), n_perms, round_hi, round_lo),
          "perm_inverse_rounds");
}
inline void fifth_root(BlsScalar *scalars, std::size_t n_scalars) {
    check(hades252_fifth_root_batch(reinterpret_cast<std::uint64_t *>(scalars), n_scalars), "fifth_root");
}
// Commitments to a matrix held column by column in host memory (include/hades252.h, CONVENTION UNPINNED like the sponge and
// the tree they are made of): scalar (r, c) = planes[c * plane_stride + r].  The row digests are those of sponge_hash on
// the transposed matrix, the tree is the one hades252_merkle_build_pad_dev writes (pad: depth digests or nullptr).  Host
// pointers only.  matrix_commit: digests and tree may be nullptr (not wanted); the root is returned.  matrix_open is plain
// host code (rows_out: n_queries x n_cols, paths_out: n_queries x depth x (arity - 1)); matrix_verify recomputes one root
// per opened row for the caller to compare.
inline void matrix_row_digests(const BlsScalar *planes, std::size_t n_rows, std::size_t n_cols, std::size_t plane_stride,
                               const BlsScalar &capacity, bool pad_one, BlsScalar *digests) {
    check(hades252_matrix_row_digests(reinterpret_cast<const std::uint64_t *>(planes), n_rows, n_cols, plane_stride,
                                      capacity.limbs, pad_one ? 1 : 0, reinterpret_cast<std::uint64_t *>(digests)),
          "matrix_row_digests");
}
inline BlsScalar matrix_commit(const BlsScalar *planes, std::size_t n_rows, std::size_t n_cols, std::size_t plane_stride,
                               const BlsScalar &capacity, bool pad_one, int arity, const BlsScalar &tag, int out_idx = 1,
                               const BlsScalar *pad = nullptr, BlsScalar *digests = nullptr, BlsScalar *tree = nullptr) {
    BlsScalar root{};
    check(hades252_matrix_commit(reinterpret_cast<const std::uint64_t *>(planes), n_rows, n_cols, plane_stride, capacity.limbs,
                                 pad_one ? 1 : 0, arity, tag.limbs, out_idx, reinterpret_cast<const std::uint64_t *>(pad),
                                 reinterpret_cast<std::uint64_t *>(digests), reinterpret_cast<std::uint64_t *>(tree), root.limbs),
          "matrix_commit");
    return root;
}
inline void matrix_open(const BlsScalar *planes, std::size_t n_rows, std::size_t n_cols, std::size_t plane_stride,
                        const BlsScalar *digests, const BlsScalar *tree, int arity, const BlsScalar *pad,
                        const std::uint64_t *indices, std::size_t n_queries, BlsScalar *rows_out, BlsScalar *paths_out) {
    check(hades252_matrix_open(reinterpret_cast<const std::uint64_t *>(planes), n_rows, n_cols, plane_stride,
                               reinterpret_cast<const std::uint64_t *>(digests), reinterpret_cast<const std::uint64_t *>(tree),
                               arity, reinterpret_cast<const std::uint64_t *>(pad), indices, n_queries,
                               reinterpret_cast<std::uint64_t *>(rows_out), reinterpret_cast<std::uint64_t *>(paths_out)),
          "matrix_open");
}
inline void matrix_verify(const BlsScalar *rows, std::size_t n_cols, const std::uint64_t *indices, const BlsScalar *paths,
                          std::size_t n_queries, int depth, int arity, const BlsScalar &capacity, bool pad_one,
                          const BlsScalar &tag, int out_idx, BlsScalar *roots) {
    check(hades252_matrix_verify(reinterpret_cast<const std::uint64_t *>(rows), n_cols, indices,
                                 reinterpret_cast<const std::uint64_t *>(paths), n_queries, depth, arity, capacity.limbs,
                                 pad_one ? 1 : 0, tag.limbs, out_idx, reinterpret_cast<std::uint64_t *>(roots)),
          "matrix_verify");
}
// The same commitment for a matrix that arrives a group of columns at a time (include/hades252.h, hades252_matstream_*): the
// row sponges stay on the device between the calls.  After absorbs of g_1, ..., g_k columns, digests and commit give what
// matrix_row_digests and matrix_commit give for the concatenated matrix and leave the stream as it is, so it can go on
// absorbing.  Host pointers only.  Movable, closes on destruction.
class MatrixStream {
    void *h_ = nullptr;
    std::size_t n_rows_ = 0;

public:
    MatrixStream(std::size_t n_rows, const BlsScalar &capacity) : n_rows_(n_rows) {
        check(hades252_matstream_open(&h_, n_rows, capacity.limbs), "MatrixStream");
    }
    MatrixStream(const MatrixStream &) = delete;
    MatrixStream &operator=(const MatrixStream &) = delete;
    MatrixStream(MatrixStream &&o) noexcept : h_(o.h_), n_rows_(o.n_rows_) { o.h_ = nullptr; o.n_rows_ = 0; }
    MatrixStream &operator=(MatrixStream &&o) noexcept {
        if (this != &o) {
            close();
            h_ = o.h_;
            n_rows_ = o.n_rows_;
            o.h_ = nullptr;
            o.n_rows_ = 0;
        }
        return *this;
    }
    ~MatrixStream() { close(); }
    void close() noexcept {
        if (h_) (void)hades252_matstream_close(h_);
        h_ = nullptr;
    }
    std::size_t n_rows() const { return n_rows_; }
    // the next n_cols columns of every row: scalar (r, j) = planes[j * plane_stride + r]
    void absorb(const BlsScalar *planes, std::size_t n_cols, std::size_t plane_stride) {
        check(hades252_matstream_absorb(h_, reinterpret_cast<const std::uint64_t *>(planes), n_cols, plane_stride),
              "MatrixStream::absorb");
    }
    std::uint64_t cols() const {
        std::uint64_t n = 0;
        check(hades252_matstream_cols(h_, &n), "MatrixStream::cols");
        return n;
    }
    void digests(bool pad_one, BlsScalar *out) {
        check(hades252_matstream_digests(h_, pad_one ? 1 : 0, reinterpret_cast<std::uint64_t *>(out)), "MatrixStream::digests");
    }
    // digests and tree may be nullptr (not wanted); the root is returned
    BlsScalar commit(bool pad_one, int arity, const BlsScalar &tag, int out_idx = 1, const BlsScalar *pad = nullptr,
                     BlsScalar *digests = nullptr, BlsScalar *tree = nullptr) {
        BlsScalar root{};
        check(hades252_matstream_commit(h_, pad_one ? 1 : 0, arity, tag.limbs, out_idx, reinterpret_cast<const std::uint64_t *>(pad),
                                        reinterpret_cast<std::uint64_t *>(digests), reinterpret_cast<std::uint64_t *>(tree),
                                        root.limbs),
              "MatrixStream::commit");
        return root;
    }
};
// Several column-major matrices of different heights under ONE tree (include/hades252.h, hades252_mmcs_*): the tree sits over
// the tallest matrix and the row digests of each shorter one are hashed into the level whose size equals its height.  absorb
// feeds the group of height n_rows (created at first use), commit is non-destructive.  Host pointers only.  Movable, frees
// on destruction.  mmcs_open is plain host code (paths_out: n_queries x depth x (arity - 1)); mmcs_verify recomputes one
// root per opening (rows: query-major, the groups' rows concatenated, tallest first) for the caller to compare.
class Mmcs {
    void *h_ = nullptr;

public:
    explicit Mmcs(const BlsScalar &capacity) { check(hades252_mmcs_new(&h_, capacity.limbs), "Mmcs"); }
    Mmcs(const Mmcs &) = delete;
    Mmcs &operator=(const Mmcs &) = delete;
    Mmcs(Mmcs &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Mmcs &operator=(Mmcs &&o) noexcept {
        if (this != &o) {
            close();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~Mmcs() { close(); }
    void close() noexcept {
        if (h_) (void)hades252_mmcs_free(h_);
        h_ = nullptr;
    }
    // the next n_cols columns of the group of height n_rows: scalar (r, j) = planes[j * plane_stride + r]
    void absorb(const BlsScalar *planes, std::size_t n_rows, std::size_t n_cols, std::size_t plane_stride) {
        check(hades252_mmcs_absorb(h_, reinterpret_cast<const std::uint64_t *>(planes), n_rows, n_cols, plane_stride),
              "Mmcs::absorb");
    }
    // columns absorbed so far for that height; 0: no such group
    std::uint64_t cols(std::size_t n_rows) const {
        std::uint64_t n = 0;
        check(hades252_mmcs_cols(h_, n_rows, &n), "Mmcs::cols");
        return n;
    }
    // tree (mmcs_tree_bytes(tallest height, arity) bytes) may be nullptr (not wanted); the root is returned
    BlsScalar commit(bool pad_one, int arity, const BlsScalar &tag, const BlsScalar &inject_tag, int out_idx = 1,
                     BlsScalar *tree = nullptr) {
        BlsScalar root{};
        check(hades252_mmcs_commit(h_, pad_one ? 1 : 0, arity, tag.limbs, inject_tag.limbs, out_idx,
                                   reinterpret_cast<std::uint64_t *>(tree), root.limbs),
              "Mmcs::commit");
        return root;
    }
    // DEVICE memory, enqueued on `stream` (include/hades252.h, f15: the caller synchronises that stream before absorb,
    // commit or the destructor run on this commitment).  n_parts column-major device matrices of distinct heights, all in
    // one launch; the four arrays are host arrays.
    void absorb_dev(const void *const *d_planes, const std::uint64_t *n_rows, const std::uint64_t *n_cols,
                    const std::uint64_t *plane_strides, std::size_t n_parts, void *stream = nullptr) {
        check(hades252_dmmcs_absorb(h_, d_planes, n_rows, n_cols, plane_strides, n_parts, stream), "Mmcs::absorb_dev");
    }
    // the device tree of the last commit (valid until the next commit or the destructor), its bytes and its arity
    const void *tree_dev(std::size_t *tree_bytes = nullptr, int *arity = nullptr) const {
        const void *tree = nullptr;
        std::size_t bytes = 0;
        int a = 0;
        check(hades252_dmmcs_tree(h_, &tree, &bytes, &a), "Mmcs::tree_dev");
        if (tree_bytes) *tree_bytes = bytes;
        if (arity) *arity = a;
        return tree;
    }
    // rows (query-major, the groups concatenated tallest first) and paths of n_queries device indices, from the committed
    // matrices (tallest first) and the tree of the last commit: what mmcs_verify_dev reads
    void open_dev(const void *const *d_planes, const std::uint64_t *n_rows, const std::uint64_t *n_cols,
                  const std::uint64_t *plane_strides, std::size_t n_parts, const std::uint64_t *d_indices, std::size_t n_queries,
                  void *d_rows, void *d_paths, void *stream = nullptr) const {
        check(hades252_dmmcs_open(h_, d_planes, n_rows, n_cols, plane_strides, n_parts, d_indices, n_queries, d_rows, d_paths,
                                  stream), "Mmcs::open_dev");
    }
    // ROW-major matrices (include/hades252.h, f16): scalar (r, j) = rows[r * row_stride + j], absorbed as the column-major
    // matrix with the same entries would be -- no transpose anywhere.  Host memory, synchronous.
    void absorb_rows(const BlsScalar *rows, std::size_t n_rows, std::size_t n_cols, std::size_t row_stride) {
        check(hades252_rmmcs_absorb_rows(h_, reinterpret_cast<const std::uint64_t *>(rows), n_rows, n_cols, row_stride),
              "Mmcs::absorb_rows");
    }
    // absorb_dev / open_dev with a layout per matrix (HADES252_LAYOUT_COLS / HADES252_LAYOUT_ROWS, a host array; nullptr:
    // all column-major): strides[p] is the plane stride or the row stride of matrix p
    void absorb_dev(const void *const *d_mats, const std::uint64_t *n_rows, const std::uint64_t *n_cols,
                    const std::uint64_t *strides, const std::uint32_t *layouts, std::size_t n_parts, void *stream = nullptr) {
        check(hades252_rmmcs_absorb_ex(h_, d_mats, n_rows, n_cols, strides, layouts, n_parts, stream), "Mmcs::absorb_dev");
    }
    void open_dev(const void *const *d_mats, const std::uint64_t *n_rows, const std::uint64_t *n_cols,
                  const std::uint64_t *strides, const std::uint32_t *layouts, std::size_t n_parts, const std::uint64_t *d_indices,
                  std::size_t n_queries, void *d_rows, void *d_paths, void *stream = nullptr) const {
        check(hades252_rmmcs_open_ex(h_, d_mats, n_rows, n_cols, strides, layouts, n_parts, d_indices, n_queries, d_rows, d_paths,
                                     stream), "Mmcs::open_dev");
    }
};
// mmcs_verify with rows, indices, paths and roots in DEVICE memory: one launch on `stream`
inline void mmcs_verify_dev(const void *d_rows, const std::uint64_t *heights, const std::uint64_t *cols, std::size_t n_groups,
                            const std::uint64_t *d_indices, const void *d_paths, std::size_t n_queries, int arity,
                            const BlsScalar &capacity, bool pad_one, const BlsScalar &tag, const BlsScalar &inject_tag, int out_idx,
                            void *d_roots, void *stream = nullptr) {
    check(hades252_dmmcs_verify(d_rows, heights, cols, n_groups, d_indices, d_paths, n_queries, arity, capacity.limbs,
                                pad_one ? 1 : 0, tag.limbs, inject_tag.limbs, out_idx, d_roots, stream),
          "mmcs_verify_dev");
}
// gadget witnesses of those openings (include/hades252.h, f17).  mmcs_perms: the permutations P of one opening's chain, 0
// for a refused shape; mmcs_steps: the chain as (kind, group, ordinal) triples, steps[3 t ..] for step t
inline std::size_t mmcs_perms(const std::uint64_t *heights, const std::uint64_t *cols, std::size_t n_groups, int arity, bool pad_one) {
    return hades252_wmmcs_perms(heights, cols, n_groups, arity, pad_one ? 1 : 0);
}
inline void mmcs_steps(const std::uint64_t *heights, const std::uint64_t *cols, std::size_t n_groups, int arity, bool pad_one,
                       std::uint32_t *steps, std::size_t n_steps) {
    check(hades252_wmmcs_steps(heights, cols, n_groups, arity, pad_one ? 1 : 0, steps, n_steps), "mmcs_steps");
}
// d_inputs: P * n_queries states of 160 B, record t * n_queries + q enters step t of opening q; d_roots may be nullptr
inline void mmcs_inputs_dev(const void *d_rows, const std::uint64_t *heights, const std::uint64_t *cols, std::size_t n_groups,
                            const std::uint64_t *d_indices, const void *d_paths, std::size_t n_queries, int arity,
                            const BlsScalar &capacity, bool pad_one, const BlsScalar &tag, const BlsScalar &inject_tag, int out_idx,
                            void *d_inputs, void *d_roots = nullptr, void *stream = nullptr) {
    check(hades252_wmmcs_inputs(d_rows, heights, cols, n_groups, d_indices, d_paths, n_queries, arity, capacity.limbs,
                                pad_one ? 1 : 0, tag.limbs, inject_tag.limbs, out_idx, d_inputs, d_roots, stream),
          "mmcs_inputs_dev");
}
// ... and d_wires: 972 * P * n_queries scalars, wire-major, exactly perm_witness of d_inputs
inline void mmcs_witness_dev(const void *d_rows, const std::uint64_t *heights, const std::uint64_t *cols, std::size_t n_groups,
                             const std::uint64_t *d_indices, const void *d_paths, std::size_t n_queries, int arity,
                             const BlsScalar &capacity, bool pad_one, const BlsScalar &tag, const BlsScalar &inject_tag, int out_idx,
                             void *d_inputs, void *d_wires, void *d_roots = nullptr, void *stream = nullptr) {
    check(hades252_wmmcs_witness(d_rows, heights, cols, n_groups, d_indices, d_paths, n_queries, arity, capacity.limbs,
                                 pad_one ? 1 : 0, tag.limbs, inject_tag.limbs, out_idx, d_inputs, d_wires, d_roots, stream),
          "mmcs_witness_dev");
}
inline std::size_t mmcs_tree_bytes(std::size_t max_rows, int arity) { return hades252_mmcs_tree_bytes(max_rows, arity); }
inline void mmcs_open(const BlsScalar *tree, std::size_t max_rows, int arity, const std::uint64_t *indices, std::size_t n_queries,
                      BlsScalar *paths_out) {
    check(hades252_mmcs_open(reinterpret_cast<const std::uint64_t *>(tree), max_rows, arity, indices, n_queries,
                             reinterpret_cast<std::uint64_t *>(paths_out)),
          "mmcs_open");
}
inline void mmcs_verify(const BlsScalar *rows, const std::uint64_t *heights, const std::uint64_t *cols, std::size_t n_groups,
                        const std::uint64_t *indices, const BlsScalar *paths, std::size_t n_queries, int arity,
                        const BlsScalar &capacity, bool pad_one, const BlsScalar &tag, const BlsScalar &inject_tag, int out_idx,
                        BlsScalar *roots) {
    check(hades252_mmcs_verify(reinterpret_cast<const std::uint64_t *>(rows), heights, cols, n_groups, indices,
                               reinterpret_cast<const std::uint64_t *>(paths), n_queries, arity, capacity.limbs, pad_one ? 1 : 0,
                               tag.limbs, inject_tag.limbs, out_idx, reinterpret_cast<std::uint64_t *>(roots)),
          "mmcs_verify");
}
// DEVICE memory, enqueued on `stream`: the whole pattern in one launch, or call by call on the 160-byte states of
// hades252_sponge_init_dev with a caller-owned cursor (0 = fresh) that moves with every call.
inline void safe_hash_dev(const void *d_in, std::size_t n_msgs, const std::uint32_t *calls, std::size_t n_calls,
                          const BlsScalar &tag, void *d_out, void *stream = nullptr) {
    check(hades252_safe_hash_dev(d_in, n_msgs, calls, n_calls, tag.limbs, d_out, stream), "safe_hash_dev");
}
inline void safe_absorb_dev(void *d_states, std::size_t n_states, const void *d_in, std::size_t len, std::uint32_t &cursor,
                            void *stream = nullptr) {
    check(hades252_safe_absorb_dev(d_states, n_states, d_in, len, &cursor, stream), "safe_absorb_dev");
}
inline void safe_squeeze_dev(void *d_states, std::size_t n_states, std::size_t len, void *d_out, std::uint32_t &cursor,
                             void *stream = nullptr) {
    check(hades252_safe_squeeze_dev(d_states, n_states, len, d_out, &cursor, stream), "safe_squeeze_dev");
}

// Gadget witnesses of permutation chains, DEVICE memory (e.g. DeviceBuffer::ptr()), enqueued on `stream`
// (include/hades252.h): permutation (s, i) is record s * n + i; d_inputs gets S * n states, d_wires 972 planes of S * n
// scalars -- what hades252_perm_witness_dev writes for those states.
inline std::size_t sponge_blocks(std::size_t msg_len, bool pad_one) { return hades252_sponge_blocks(msg_len, pad_one ? 1 : 0); }

inline void sponge_witness(const void *d_msgs, std::size_t n_msgs, std::size_t msg_len, const BlsScalar &capacity, bool pad_one,
                           void *d_inputs, void *d_wires, void *d_digests = nullptr, void *stream = nullptr) {
    check(hades252_sponge_witness_dev(d_msgs, n_msgs, msg_len, capacity.limbs, pad_one ? 1 : 0, d_inputs, d_wires, d_digests,
                                      stream), "sponge_witness");
}

inline void merkle_open_witness(const void *d_leaves, const void *d_tree, std::size_t n_leaves, int arity, const BlsScalar &tag,
                                const void *d_pad, const std::uint64_t *d_indices, std::size_t n_queries, void *d_inputs,
                                void *d_wires, int *d_bad_count = nullptr, void *stream = nullptr) {
    check(hades252_merkle_open_witness_dev(d_leaves, d_tree, n_leaves, arity, tag.limbs, d_pad, d_indices, n_queries, d_inputs,
                                           d_wires, d_bad_count, stream), "merkle_open_witness");
}

// The cipher's gadget witnesses (same device conventions): S = cipher_perms(msg_len) records per message; the side outputs
// (ciphers, or messages + verdicts + a device rejection counter) may be nullptr.
inline std::size_t cipher_perms(std::size_t msg_len) { return hades252_cipher_perms(msg_len); }

inline void cipher_encrypt_witness(const void *d_msgs, const void *d_keys, const void *d_nonces, std::size_t n_msgs,
                                   std::size_t msg_len, const BlsScalar &domain, void *d_inputs, void *d_wires,
                                   void *d_ciphers = nullptr, void *stream = nullptr) {
    check(hades252_cipher_encrypt_witness_dev(d_msgs, d_keys, d_nonces, n_msgs, msg_len, domain.limbs, d_inputs, d_wires,
                                              d_ciphers, stream), "cipher_encrypt_witness");
}

inline void cipher_decrypt_witness(const void *d_ciphers, const void *d_keys, const void *d_nonces, std::size_t n_msgs,
                                   std::size_t msg_len, const BlsScalar &domain, void *d_inputs, void *d_wires,
                                   void *d_msgs = nullptr, std::uint8_t *d_ok = nullptr, int *d_rejected = nullptr,
                                   void *stream = nullptr) {
    check(hades252_cipher_decrypt_witness_dev(d_ciphers, d_keys, d_nonces, n_msgs, msg_len, domain.limbs, d_inputs, d_wires,
                                              d_msgs, d_ok, d_rejected, stream), "cipher_decrypt_witness");
}

// The duplex sponge with its records: the whole pattern (S = safe_pattern(..).n_perms steps; d_out may be nullptr), or
// call by call -- safe_absorb_dev / safe_squeeze_dev that also record the permutations they run as steps step, step + 1, ..
// of buffers sized for total_steps steps; `step` moves with every call, like the cursor.
inline void safe_witness(const void *d_in, std::size_t n_msgs, const std::uint32_t *calls, std::size_t n_calls,
                         const BlsScalar &tag, void *d_inputs, void *d_wires, void *d_out = nullptr, void *stream = nullptr) {
    check(hades252_safe_witness_dev(d_in, n_msgs, calls, n_calls, tag.limbs, d_inputs, d_wires, d_out, stream),
          "safe_witness");
}
inline void safe_absorb_witness_dev(void *d_states, std::size_t n_states, const void *d_in, std::size_t len,
                                    std::uint32_t &cursor, void *d_inputs, void *d_wires, std::size_t total_steps,
                                    std::size_t &step, void *stream = nullptr) {
    check(hades252_safe_absorb_witness_dev(d_states, n_states, d_in, len, &cursor, d_inputs, d_wires, total_steps, &step,
                                           stream), "safe_absorb_witness_dev");
}
inline void safe_squeeze_witness_dev(void *d_states, std::size_t n_states, std::size_t len, void *d_out,
                                     std::uint32_t &cursor, void *d_inputs, void *d_wires, std::size_t total_steps,
                                     std::size_t &step, void *stream = nullptr) {
    check(hades252_safe_squeeze_witness_dev(d_states, n_states, len, d_out, &cursor, d_inputs, d_wires, total_steps, &step,
                                            stream), "safe_squeeze_witness_dev");
}

// What the library caches (pipes: streams, chunk buffers, staging memory) and which kernel a batch size gets.
inline void trim() { check(hades252_trim(), "trim"); }
inline std::size_t pool_bytes() { return hades252_pool_bytes(); }
/// Pay the one-time costs (code object, pipe for a host batch of `n_perms_hint` states) before the first real call.
inline void warm_up(std::size_t n_perms_hint = 0) { check(hades252_warm_up(n_perms_hint), "warm_up"); }
inline int kernel_for(std::size_t n_perms) { return hades252_kernel_for(n_perms); }
inline const char *kernel_name(int kernel, std::size_t n_perms) { return hades252_kernel_name(kernel, n_perms); }

}  // namespace dusk_hades
#endif
