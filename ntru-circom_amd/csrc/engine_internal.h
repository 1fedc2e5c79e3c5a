// engine_internal.h -- what the translation units of libntru_engine.so share (not part of the C ABI).
//
//   abi.hip                  engine life cycle + the *_dev entry points that choose between kernel families
//   valu_families.hip        vector-ALU families 1-3 (one ciphertext per wavefront): MAC, ternary add path, shared stepping + dot8
//   matrix_encrypt.hip       family 4, encryptBits with a shared key on the int8 matrix cores (k_encrypt_m, k_encrypt_md)
//   matrix_decrypt.hip       family 4, decryptBits with a shared key (k_decrypt_m, k_decrypt_m8)
//   matrix_peritem.hip       family 4 with per-item operands (k_verify_keys_m, k_polymul_m, k_product_tern_m)
//   key_inversion.hip        key inversion: k_invert_key, the Newton rounds around the per-item product kernels, ntru_invert_key_batch_dev
//   ternary_sampler.hip      the on-device ternary sampler: k_sample_ternary for consecutive or listed stream positions, its launchers,
//                            ntru_sample_ternary_dev
//   elementwise.hip          split by I, add, field packing and unpacking (kernels and *_dev entry points), ntru_pack_params
//   ntru_host.hip            host-pointer entry points: every regular one (its _dev form through the chunked H2D / kernel / D2H pipeline below,
//                            from one description per call) with its ntru_multi_ form, ntru_pipeline_batch, device buffers; no kernels
//   ntru_generic.hip         reference-faithful generic family (arbitrary divisors, moduli up to 2^26, signed coefficients)
//   witness_check.hip        witness checks against the Verify* circuits (kernels and *_dev entry points)
//   keygen_batch.hip         batched key generation with on-device redraws (kernels, *_dev and host-pointer entry points)
//   ciphertext_sum.hip       segmented, weighted sums of ciphertext rows + tally decrypt (kernels, *_dev and host-pointer entry points)
//   message_bytes.hip        byte messages as packed bits: bytes <-> coefficient rows, encrypt / decrypt / pipeline on bytes (kernels, *_dev
//                            entry points and ntru_pipeline_bytes_batch)
//   packed_ciphertexts.hip   ciphertexts as packOutput(q - 1, N, e) rows: sums straight from the packed rows, unpack to dense rows, tally
//                            and decrypt on them (kernels, *_dev and host-pointer entry points)
//   matrix_reencrypt.hip     re-randomising and shuffling ciphertexts: the shared-key encrypt body (matrix_encrypt_body.h) with a gathered
//                            16-bit row as the addend (k_reencrypt_m, k_reencrypt_md), the add kernel behind the vector-ALU route, the *_dev
//                            and host-pointer entry points
//   scan_hits.hip            scanning a batch for the rows a key decrypts to a well-formed, tagged message: decrypt and rows_to_bytes as
//                            they are, then mark / offsets / emit kernels that compact the hits on the device (kernels, *_dev and
//                            host-pointer entry points)
//   permutation.hip          the order of a mix step drawn on the device: ChaCha20 sort keys (k_perm_keys), a stable radix argsort without
//                            global atomics (k_perm_hist / k_perm_offsets / k_perm_scatter per byte, k_perm_finish), and a whole mix step
//                            from a key: sample r, draw the order, re-encrypt (kernels, *_dev and host-pointer entry points)
//   matrix_combine.hip       G linear combinations of the same rows by a weight matrix, out = W^T rows: the contraction over the batch axis on
//                            the int8 matrix cores (k_combine_m), the vector-ALU twin (k_combine_v), the finish over row blocks (kernels, *_dev
//                            and host-pointer entry points)
//   matrix_mulshared.hip     a batch of full-range rows times ONE full-range polynomial, with the split: batch x Toeplitz matrix on the int8
//                            matrix cores with both operands in two digit planes (k_mul_shared_m), the replicated per-item route for
//                            everything outside its range (kernel, *_dev and host-pointer entry points)
//   matrix_noise.hip         the decryption noise of rows under one key: decrypt's first product on the int8 matrix cores reduced to
//                            peak and energy in the epilogue (k_noise_m), the vector-ALU decrypt's rem1 reduced pass by pass for
//                            everything outside its range (k_noise_rows), dense and packed rows (kernels, *_dev and host-pointer entry
//                            points)
//   dedup_rows.hip           the duplicate rows of a batch, dense or packed, against an optional prior set: keyed 64-bit fingerprints
//                            (k_dedup_fingerprint), permutation.hip's stable argsort, one exact comparison with the sorted
//                            predecessor (k_dedup_neighbours), a walk for true collisions only (k_dedup_walk), prefix-sum compaction
//                            (kernels, *_dev and host-pointer entry points)
//   count_bytes.hip          the decrypted byte messages of a batch counted by choice and group: decrypt and rows_to_bytes as they
//                            are, then one classifying kernel (k_count_classify) that counts in an LDS histogram or, for large
//                            tables, with one global atomic per row (kernel, *_dev and host-pointer entry points)
// Every kernel family exports the host function that launches it (ntru_launch_*, hidden visibility); a launcher returns
// NTRU_NOT_TAKEN when the parameters are outside its family's range and the dispatcher in abi.hip tries the next one.
#ifndef NTRU_ENGINE_INTERNAL_H
#define NTRU_ENGINE_INTERNAL_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ntru_engine.h"

#define NTRU_HIDDEN __attribute__((visibility("hidden")))

// Per-thread message behind ntru_last_error(); returns `code`.
NTRU_HIDDEN int ntru_fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return ntru_fail(NTRU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
  } while (0)

// A buffer that only grows: allocated on first use, reused by every later call, released with the engine.
struct GrowBuf {
  void *p = nullptr;
  size_t cap = 0;
};

// Host-path staging (ntru_host.hip): a chunk moves through three STAGES, each with its own engine-owned stream -- upload (H2D),
// compute (the *_dev launches), download (D2H) -- chained by events, so that at any time ONE upload, one set of kernels and ONE
// download are in flight: chunk k+1 goes up while chunk k computes and chunk k-1 comes down (PCIe is full duplex: 57 GB/s one
// way, 47 + 47 GB/s both ways on this box, profiles/archive/r03_pcie_duplex.json).  Chunk k owns buffer set k % 3 (pinned host arena +
// device arena + scratch) until its download has finished.  [Round 2 ran each chunk on the stream of one of TWO slots: the two
// slots fell into lock-step -- both uploading, then both computing, then both downloading -- and the two directions never
// overlapped: 56 GB/s in total.]
struct HostSlot {
  GrowBuf pinned;           // hipHostMalloc
  GrowBuf dev;              // hipMalloc
  GrowBuf scratch;          // temporaries of a *_dev call of the chunk that owns this set
  hipEvent_t up_done = nullptr, comp_done = nullptr, down_done = nullptr;
  bool busy = false;        // a chunk has been enqueued with this set and its download has not been waited for yet
};
constexpr int NTRU_HOST_SLOTS = 3;

struct ntru_engine {
  int device;
  hipStream_t stream;       // caller's stream for the *_dev entry points (never owned)
  int cus;
  int path;                 // ntru_engine_set_kernel_path: 0 auto, 1 MAC kernels, 2 add path, 3 add path without dot8, 4 matrix cores as two
                            // workgroups per CU, 5 matrix cores with the lock-step decrypt
  int sampler_rounds;       // ntru_engine_set_sampler_rounds: 20 (RFC 8439, default), 12 or 8 rounds of the sampler's ChaCha block function
  int lift;                 // ntru_engine_set_lift: NTRU_LIFT_REFERENCE (default) or NTRU_LIFT_CENTRED; the decrypt launchers read it
  char last_kernel[64];     // name of the kernel the last *_dev call launched (reporting only)
  HostSlot slot[NTRU_HOST_SLOTS];
  hipStream_t st_up, st_comp, st_down;   // the three stage streams of the host path (created at first use)
  hipStream_t st_aux;       // forked from / joined back into the caller's stream inside ONE *_dev call (key inversion: the mod-p inversion,
  hipEvent_t ev_fork, ev_join;   // vector-ALU bound, runs beside the Newton chain on the matrix cores); created at first use
  GrowBuf shared_dev;       // what ONE host form keeps on the device across the chunks of its Pipeline run (sums and offsets, combined
                            // rows, scan counts and hits, a drawn order); taken through ResidentHold only
  const char *shared_holder = nullptr;   // the host form that holds shared_dev now (ResidentHold), or NULL
  GrowBuf scratch_dev;      // temporaries of *_dev calls (Newton rounds, generic family) on the caller's stream
  GrowBuf keygen_work;      // workspace of the host-pointer ntru_keygen_batch (ntru_keygen_workspace_bytes of one chunk)
  hipStream_t scratch_stream;   // the stream whose work used scratch_dev last, and an event recorded behind that work: a call on
  hipEvent_t scratch_event;     // ANOTHER stream waits for it before it touches the buffer (ntru_scratch_acquire / _release)
  bool scratch_used;
  GrowBuf *cur_scratch;     // = &scratch_dev, or a slot's scratch while the host path borrows the engine for that slot
  // (kernel function, LDS bytes, block size) -> co-resident blocks per CU, filled at first use
  struct OccEntry { const void *fn; size_t lds; int threads; int per_cu; };
  OccEntry occ[64];
  int n_occ;
};

// Grows `b` to at least `bytes` of device memory (contents are not preserved).  Growing frees the old buffer, and hipFree waits
// for the whole device.
NTRU_HIDDEN int ntru_grow_dev(GrowBuf *b, size_t bytes);
// Grows `b` to at least `bytes` of pinned host memory.
NTRU_HIDDEN int ntru_grow_pinned(GrowBuf *b, size_t bytes);
// hipOccupancyMaxActiveBlocksPerMultiprocessor, cached per engine.
NTRU_HIDDEN int ntru_blocks_per_cu(ntru_engine *eng, const void *fn, int threads, size_t lds, int *per_cu);
// eng->cur_scratch grown to `bytes` for work about to be enqueued on eng->stream.  If the previous user of the engine-owned
// buffer ran on another stream, eng->stream first waits for that work (two *_dev calls on different streams no longer race).
NTRU_HIDDEN int ntru_scratch_acquire(ntru_engine *eng, size_t bytes, char **p);
// Marks the end of the work enqueued since ntru_scratch_acquire (records the event the next other-stream user waits for).
NTRU_HIDDEN int ntru_scratch_release(ntru_engine *eng);

// Scope guard around the two calls above: acquires now, releases on EVERY way out of the caller (an early error return must still
// record the event: kernels that are already enqueued keep using the buffer, and the next call on another stream has to wait for them).
struct ScratchHold {
  ntru_engine *eng;
  char *p = nullptr;
  int rc;
  ScratchHold(ntru_engine *e, size_t bytes) : eng(e) { rc = ntru_scratch_acquire(e, bytes, &p); }
  ~ScratchHold() { if (rc == NTRU_OK) (void)ntru_scratch_release(eng); }
  ScratchHold(const ScratchHold &) = delete;
  ScratchHold &operator=(const ScratchHold &) = delete;
};

// ---- host helpers shared by the translation units ---------------------------------------------------------------------------
#define NTRU_NOT_TAKEN (-1000)      // a launcher's "not my parameter range"; never leaves the library

static inline int fail(int code, const std::string &msg) { return ntru_fail(code, msg); }
static inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
// Bytes rounded up to the 256-byte granule at which scratch, workspace and staging arrays are carved.
static inline size_t ntru_up256(size_t v) { return (v + 255) & ~(size_t)255; }
// Arrays carved out of one buffer, one after the other at that granule: take(bytes) is where the next array starts, `total` what
// has been taken so far.
struct NTRU_HIDDEN Carve {
  size_t total = 0;
  size_t take(size_t bytes) {
    const size_t at = total;
    total += ntru_up256(bytes);
    return at;
  }
};

// eng->shared_dev grown to `bytes` and held by the host form `what` until the guard leaves scope.  Growing frees the old buffer, so a
// host form that holds it must not call another that takes it: the second hold fails (NTRU_ERR_ARG, both names) and grows nothing.
struct NTRU_HIDDEN ResidentHold {
  ntru_engine *eng;
  char *p = nullptr;
  int rc;
  ResidentHold(ntru_engine *e, const char *what, size_t bytes) : eng(e) {
    if (e->shared_holder) {
      rc = ntru_fail(NTRU_ERR_ARG, std::string(what) + ": the engine's resident buffer is held by " + e->shared_holder);
      return;
    }
    if ((rc = ntru_grow_dev(&e->shared_dev, bytes))) return;
    e->shared_holder = what;
    p = (char *)e->shared_dev.p;
  }
  ~ResidentHold() { if (rc == NTRU_OK) eng->shared_holder = nullptr; }
  ResidentHold(const ResidentHold &) = delete;
  ResidentHold &operator=(const ResidentHold &) = delete;
};

// f(first row, rows) for consecutive passes of at most `pass` rows over B rows; the first non-zero return ends the walk.
template <class F>
static inline int for_each_pass(int64_t B, int64_t pass, F f) {
  for (int64_t o = 0; o < B; o += pass)
    if (int rc = f(o, std::min<int64_t>(pass, B - o))) return rc;
  return NTRU_OK;
}
// An optional array `elems` elements on.
template <class T>
static inline T *rows_at(T *p, int64_t elems) { return p ? p + elems : nullptr; }

// Whether [a, a + na) and [b, b + nb) share a byte; nothing overlaps a NULL pointer or an empty range.
static inline bool ntru_ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// One chunk's share of `rows` result rows that several chunks add up: launch(dst) enqueues it; the first chunk stores into d_out, every
// later one stores beside it in d_tmp and adds.
template <class Launch>
static inline int accumulate_chunk(ntru_engine *eng, int N, int mod, bool first, int64_t rows, uint16_t *d_out, uint16_t *d_tmp,
                                   Launch launch) {
  if (int rc = launch(first ? d_out : d_tmp)) return rc;
  return first ? (int)NTRU_OK : ntru_add_batch_dev(eng, N, mod, d_out, d_tmp, rows, d_out);
}

// (N, mod) of the sums and combinations of rows; `who` ends where the message begins ("name: ").
static inline int ntru_check_ring_mod(const std::string &who, int N, int mod) {
  if (N < 2 || N > NTRU_MAX_N) return fail(NTRU_ERR_ARG, who + "need 2 <= N <= " + std::to_string(NTRU_MAX_N) + ", got N = " + std::to_string(N));
  if (mod < 2 || mod > 65536) return fail(NTRU_ERR_ARG, who + "need 2 <= mod <= 65536, got " + std::to_string(mod));
  return NTRU_OK;
}

// What ntru_engine_last_kernel() reports: a plain name, or a templated family's name<K> / name<K,me> (me < 0: no second argument).
static inline void note_kernel(ntru_engine *eng, const char *name) { snprintf(eng->last_kernel, sizeof eng->last_kernel, "%s", name); }
static inline void note_kernel(ntru_engine *eng, const char *family, int K, int me) {
  if (me >= 0) snprintf(eng->last_kernel, sizeof eng->last_kernel, "%s<%d,%d>", family, K, me);
  else snprintf(eng->last_kernel, sizeof eng->last_kernel, "%s<%d>", family, K);
}
// Workgroups of 256 for an elementwise kernel.  Kernels that move 16 bytes per lane and access (streaming = true) get TWO per CU: more
// resident waves lower the HBM rate (the add of two ciphertext batches: 5.0 TB/s with 8 per CU, 5.9 with 2, 4.8 with 1:
// profiles/archive/r03_ab_elementwise_grid.txt); element-per-lane kernels keep 8.
static inline dim3 elementwise_grid(const ntru_engine *eng, long total, bool streaming = false) {
  const int per_cu = streaming ? 2 : 8;
  long blocks = (total + 255) / 256, cap = (long)eng->cus * per_cu;
  return dim3((unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks)));
}
// What decryptBits' lift adds to x > q/2 before the reduction mod p: index.js:117's 1, or -q mod p in NTRU_LIFT_CENTRED.  Read when a
// call enqueues, handed to the kernel by value.
static inline uint32_t ntru_lift_addend(const ntru_engine *eng, int q, int p) {
  return eng->lift == NTRU_LIFT_CENTRED ? (uint32_t)((p - q % p) % p) : 1u;
}
// (N, q, B) of the packed kernels: q a power of two <= 65536, 2 <= N <= NTRU_MAX_N
NTRU_HIDDEN int ntru_check_common(const ntru_engine *eng, int N, int q, long B);
// p of decryptBits and of the key checks: a small modulus that is no power of two, N*(p-1)^2 < 65536
NTRU_HIDDEN int ntru_check_decrypt_p(int N, int p);

// ---- launchers (defined next to their kernels) --------------------------------------------------------------------------------
// encryptBits / decryptBits with a shared key on the matrix cores; rows at a pitch of ld elements
NTRU_HIDDEN int ntru_launch_encrypt_matrix(ntru_engine *eng, int N, int q, int ld, const uint16_t *d_h, const uint8_t *d_r,
                                           const uint8_t *d_m, int64_t B, uint16_t *d_e, uint16_t *d_quotE);
NTRU_HIDDEN int ntru_launch_decrypt_matrix(ntru_engine *eng, int N, int q, int p, int ld, const int8_t *d_f, const uint8_t *d_fp,
                                           const uint16_t *d_e, int64_t B, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1,
                                           uint8_t *d_quot2);
// decryptBits + packOutput(p - 1, N, value) in one kernel; d_value may be NULL (NTRU_NOT_TAKEN outside the matrix path's range)
NTRU_HIDDEN int ntru_launch_decrypt_pack_matrix(ntru_engine *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                                const uint16_t *d_e, int64_t B, uint8_t *d_value, uint64_t *d_packed, int out_size);
// encryptBits + packOutput on the row-image kernel (matrix_rowimage.hip): dense rows, one eight-wave workgroup per CU, results leave
// through an LDS image
NTRU_HIDDEN int ntru_launch_encrypt_pack_rowimage(ntru_engine *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, const uint8_t *d_m,
                                                  int64_t B, uint64_t *d_packed, int os);
// the same on the vector-ALU families (dense rows); never NTRU_NOT_TAKEN
NTRU_HIDDEN int ntru_launch_encrypt_valu(ntru_engine *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, const uint8_t *d_m,
                                         int64_t B, uint16_t *d_e, uint16_t *d_quotE);
NTRU_HIDDEN int ntru_launch_decrypt_valu(ntru_engine *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                         const uint16_t *d_e, int64_t B, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1,
                                         uint8_t *d_quot2);
// per-item products
// one Newton round of the key inversion (v from kb to m bits) as one kernel; _applies: kb <= 7, kb < m <= 2 kb, per-item matrix range
NTRU_HIDDEN bool ntru_newton_round_matrix_applies(const ntru_engine *eng, int N, int kb, int m);
NTRU_HIDDEN int ntru_launch_newton_round_matrix(ntru_engine *eng, int N, int kb, int m, const int8_t *d_f, uint16_t *d_v, long B);
NTRU_HIDDEN int ntru_launch_polymul_matrix(ntru_engine *eng, int N, int mod, const uint16_t *d_a, const uint16_t *d_b, int64_t B,
                                           uint16_t *d_quot, uint16_t *d_rem);
NTRU_HIDDEN int ntru_launch_polymul_valu(ntru_engine *eng, int N, int mod, const uint16_t *d_a, const uint16_t *d_b, int64_t B,
                                         uint16_t *d_quot, uint16_t *d_rem);
NTRU_HIDDEN bool ntru_product_tern_matrix_applies(const ntru_engine *eng, int N, int q);
// ((mul * a) mod q) * s with s ternary per item; d_quot may be NULL
NTRU_HIDDEN int ntru_launch_product_tern_matrix(ntru_engine *eng, int N, int q, uint32_t mul, const uint16_t *d_a, const int8_t *d_s,
                                                long B, uint16_t *d_rem);
NTRU_HIDDEN int ntru_launch_public_key_valu(ntru_engine *eng, int N, int q, int p, const uint16_t *d_fq, const int8_t *d_g, int64_t B,
                                            uint16_t *d_h);
NTRU_HIDDEN int ntru_launch_verify_keys_matrix(ntru_engine *eng, int N, int q, int p, const int8_t *d_f, const int8_t *d_g,
                                               const uint16_t *d_fq, const uint8_t *d_fp, const uint16_t *d_h, int64_t B,
                                               uint16_t *d_quot_fq, uint16_t *d_rem_fq, uint8_t *d_quot_fp, uint8_t *d_rem_fp,
                                               uint16_t *d_quot_h, uint16_t *d_rem_h, uint8_t *d_flags);
NTRU_HIDDEN int ntru_launch_verify_keys_valu(ntru_engine *eng, int N, int q, int p, const int8_t *d_f, const int8_t *d_g,
                                             const uint16_t *d_fq, const uint8_t *d_fp, const uint16_t *d_h, int64_t B,
                                             uint16_t *d_quot_fq, uint16_t *d_rem_fq, uint8_t *d_quot_fp, uint8_t *d_rem_fp,
                                             uint16_t *d_quot_h, uint16_t *d_rem_h, uint8_t *d_flags);

// k_sample_ternary (ternary_sampler.hip) for the items d_idx[0 .. n) of a device list: compact row k is the row of stream position
// pos_base + d_idx[k] under `key` (eight words).  Always ChaCha20; N + 1 < 2048.
NTRU_HIDDEN int ntru_launch_sample_listed(ntru_engine *eng, int N, int n1, int n2, int other, const uint32_t *key, uint64_t pos_base,
                                          const uint32_t *d_idx, int n, uint8_t *d_out);

// ---- sums of rows in groups (ciphertext_sum.hip; packed_ciphertexts.hip sums packed rows through the same finish kernel and host form)
// The groups of one launch as the host hands them on: off != NULL (DEVICE, G + 1 row indices): group g is rows [off[g], off[g + 1]);
// else rows [(g0 + g) K, (g0 + g + 1) K); both clamped to the window [wlo, whi), whose first row is the first row of the array passed.
struct SumWindow {
  const int64_t *off;
  int64_t K, g0, G, wlo, whi;
};
// Enqueues the sums of the groups `w` of the rows at d_rows (dense uint16_t rows or packed rows) into d_out [w.G][N].
typedef int (*ntru_sum_launcher)(ntru_engine *eng, int N, int mod, const void *d_rows, const uint16_t *d_weights, const SumWindow &w,
                                 uint16_t *d_out);
// the domain and argument checks of ntru_sum_groups under the name `who`
NTRU_HIDDEN int ntru_check_sum_args(const ntru_engine *eng, int N, int mod, bool uniform, int64_t K, int64_t G, const char *who);
// k_sum_groups_finish on the partial rows a row kernel left for Pb row blocks, in the scratch that launch_sum_rows sized and carved
// (sum_groups_common.h: the one launcher of both row kernels; the body of the four tally calls is there too); nothing to do for Pb == 1
NTRU_HIDDEN int ntru_launch_sum_finish(ntru_engine *eng, int N, int mod, const SumWindow &w, long Pb, const uint32_t *d_part,
                                       const long *d_meta, uint16_t *d_out);
// The host-pointer form of a sum: validates offsets and weights, streams the rows (row_bytes each) through the chunked pipeline, one
// window of rows per chunk, and accumulates a group larger than a chunk across chunks.
NTRU_HIDDEN int ntru_sum_groups_host(ntru_engine *eng, const char *who, int N, int mod, const void *rows, size_t row_bytes,
                                     const uint16_t *weights, const int64_t *offsets, int64_t K, int64_t G, uint16_t *out,
                                     ntru_sum_launcher launch);

// ---- packed rows (packed_ciphertexts.hip) -----------------------------------------------------------------------------------------------
// Enqueues k_unpack_rows: B rows of packOutput(q - 1, N, e) -> dense uint16_t [B][N] (scan_hits.hip unpacks a pass with it).
NTRU_HIDDEN int ntru_launch_unpack_rows(ntru_engine *eng, int N, int q, const uint64_t *d_packed, int64_t B, uint16_t *d_rows);

// ---- re-randomising from host pointers (matrix_reencrypt.hip) -------------------------------------------------------------------------------
// Where the rows of r come from when the caller does not supply them: row i is row 0 of ntru_sample_ternary_dev(N, n1, n2, other, key,
// first_item + i, 1), drawn on the device; r_out (host, [B][N], may be NULL) receives them.
struct ReencryptDraw {
  const uint32_t *key;
  uint64_t first_item;
  int n1, n2, other;
  uint8_t *r_out;
};
// The body of ntru_reencrypt_batch; with r == NULL the rows of r come from `draw` (ntru_mix_batch, permutation.hip).
NTRU_HIDDEN int ntru_reencrypt_host(ntru_engine *eng, int N, int q, const uint16_t *h, const uint8_t *r, const ReencryptDraw *draw,
                                    const uint16_t *e_in, int64_t B_in, const int64_t *src, int64_t B, uint16_t *e_out, uint16_t *quotE);

// ---- host-pointer entry points (ntru_host.hip; keygen_batch, ciphertext_sum, message_bytes) --------------------------------------------------------------
// True when `p` points into memory HIP knows as pinned host memory (hipHostMalloc / hipHostRegister).
NTRU_HIDDEN bool ntru_is_pinned(const void *p);
// memcpy on several threads once the block is large enough for the extra threads to pay for themselves.
NTRU_HIDDEN void ntru_big_memcpy(void *dst, const void *src, size_t bytes);
// Items per chunk of a Pipeline run.
NTRU_HIDDEN int64_t ntru_chunk_items(int64_t B);

// The chunked H2D / compute / D2H pipeline behind every host-pointer entry point: declare the arrays (in / out / tmp), then run()
// calls launch(first item, items, device pointers in declaration order) once per chunk on eng->stream.
struct Pipeline {
  static constexpr int MAX_ARR = 16;
  struct HArr {
    const void *src = nullptr;   // host source (inputs)
    void *dst = nullptr;         // host destination (outputs); an output with dst == nullptr is not wanted
    size_t row = 0;              // bytes per item, or total bytes when `shared`
    bool shared = false;         // the same bytes for every chunk (key rows)
    bool direct = false;         // host memory is pinned: DMA straight from / to it
    bool temp = false;           // lives on the device only (an intermediate of a multi-stage chunk): no copy either way
    size_t dev_off = 0, pin_off = 0;
  };
  struct Pending { void *dst; const void *pin; size_t bytes; };

  ntru_engine *eng;
  HArr arr[MAX_ARR];
  int n = 0;
  std::vector<Pending> pending[NTRU_HOST_SLOTS];
  hipStream_t saved_stream;
  GrowBuf *saved_scratch;

  explicit Pipeline(ntru_engine *e) : eng(e), saved_stream(e->stream), saved_scratch(e->cur_scratch) {}
  ~Pipeline() { eng->stream = saved_stream; eng->cur_scratch = saved_scratch; }

  int in(const void *p, size_t row, bool shared = false) {
    arr[n].src = p; arr[n].row = row; arr[n].shared = shared; arr[n].direct = !shared && ntru_is_pinned(p);
    return n++;
  }
  int out(void *p, size_t row) {
    arr[n].dst = p; arr[n].row = row; arr[n].direct = p && ntru_is_pinned(p);
    return n++;
  }
  int tmp(size_t row) {          // device-only rows of a chunk (what one stage hands the next)
    arr[n].row = row; arr[n].temp = true;
    return n++;
  }

  // Waits until the chunk that owns buffer set s has been downloaded, then hands its staged outputs to the caller's arrays.
  int drain(int s) {
    HostSlot &sl = eng->slot[s];
    if (!sl.busy) return NTRU_OK;
    HIP_TRY(hipEventSynchronize(sl.down_done));
    sl.busy = false;
    for (const Pending &p : pending[s]) ntru_big_memcpy(p.dst, p.pin, p.bytes);
    pending[s].clear();
    return NTRU_OK;
  }

  // launch(first item, items, device pointers in the order the arrays were declared) enqueues on eng->stream.
  template <class F>
  int run(int64_t B, int64_t C, F launch) {
    HIP_TRY(hipSetDevice(eng->device));
    if (C > B) C = B;
    if (C < 1) C = 1;
    size_t dev_bytes = 0, pin_bytes = 0;
    for (int i = 0; i < n; i++) {
      HArr &a = arr[i];
      const size_t bytes = a.shared ? a.row : a.row * (size_t)C;
      if (!a.src && !a.dst && !a.temp) continue;
      a.dev_off = dev_bytes; dev_bytes += ntru_up256(bytes);
      if (!a.direct && !a.temp) { a.pin_off = pin_bytes; pin_bytes += ntru_up256(bytes); }
    }
    for (hipStream_t *st : {&eng->st_up, &eng->st_comp, &eng->st_down})
      if (!*st) HIP_TRY(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    const int64_t nchunks = (B + C - 1) / C;
    // A single chunk (every call of the reference's own API) has nothing to overlap with: its three stages go onto ONE stream, in
    // order, without events between them.
    const bool single = nchunks == 1;
    const hipStream_t s_up = single ? eng->st_comp : eng->st_up, s_down = single ? eng->st_comp : eng->st_down;
    for (int s = 0; s < NTRU_HOST_SLOTS && s < nchunks; s++) {          // a single chunk touches one buffer set only
      HostSlot &sl = eng->slot[s];
      for (hipEvent_t *ev : {&sl.up_done, &sl.comp_done, &sl.down_done})
        if (!*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
      if (int rc = ntru_grow_dev(&sl.dev, dev_bytes)) return rc;
      if (int rc = ntru_grow_pinned(&sl.pinned, pin_bytes)) return rc;
    }
    int rc = NTRU_OK;
    int64_t k = 0;
    for (int64_t o = 0; o < B && rc == NTRU_OK; o += C, k++) {
      const int s = (int)(k % NTRU_HOST_SLOTS);
      const int64_t cnt = std::min(C, B - o);
      HostSlot &sl = eng->slot[s];
      if ((rc = drain(s))) break;                        // chunk k - 3 is out of this buffer set
      // ---- stage 1: upload (staging copies on this thread, DMA on the upload stream)
      void *dev[MAX_ARR];
      for (int i = 0; i < n && rc == NTRU_OK; i++) {
        HArr &a = arr[i];
        dev[i] = (a.src || a.dst || a.temp) ? (char *)sl.dev.p + a.dev_off : nullptr;
        if (!a.src) continue;
        const size_t bytes = a.shared ? a.row : a.row * (size_t)cnt;
        const char *from = (const char *)a.src + (a.shared ? 0 : a.row * (size_t)o);
        if (!a.direct) {
          char *pin = (char *)sl.pinned.p + a.pin_off;
          ntru_big_memcpy(pin, from, bytes);
          from = pin;
        }
        if (hipMemcpyAsync(dev[i], from, bytes, hipMemcpyHostToDevice, s_up) != hipSuccess)
          rc = ntru_fail(NTRU_ERR_HIP, "hipMemcpyAsync (host to device) failed");
      }
      if (!single && rc == NTRU_OK && hipEventRecord(sl.up_done, s_up) != hipSuccess) rc = ntru_fail(NTRU_ERR_HIP, "hipEventRecord failed");
      // ---- stage 2: compute, behind this chunk's upload
      if (!single && rc == NTRU_OK && hipStreamWaitEvent(eng->st_comp, sl.up_done, 0) != hipSuccess) rc = ntru_fail(NTRU_ERR_HIP, "hipStreamWaitEvent failed");
      eng->stream = eng->st_comp;
      eng->cur_scratch = &sl.scratch;
      if (rc == NTRU_OK) rc = launch(o, cnt, dev);
      if (!single && rc == NTRU_OK && hipEventRecord(sl.comp_done, eng->st_comp) != hipSuccess) rc = ntru_fail(NTRU_ERR_HIP, "hipEventRecord failed");
      // ---- stage 3: download, behind this chunk's kernels
      if (!single && rc == NTRU_OK && hipStreamWaitEvent(s_down, sl.comp_done, 0) != hipSuccess) rc = ntru_fail(NTRU_ERR_HIP, "hipStreamWaitEvent failed");
      for (int i = 0; i < n && rc == NTRU_OK; i++) {
        HArr &a = arr[i];
        if (!a.dst) continue;
        const size_t bytes = a.row * (size_t)cnt;
        char *to = (char *)a.dst + a.row * (size_t)o;
        if (!a.direct) {
          char *pin = (char *)sl.pinned.p + a.pin_off;
          pending[s].push_back({to, pin, bytes});
          to = pin;
        }
        if (hipMemcpyAsync(to, dev[i], bytes, hipMemcpyDeviceToHost, s_down) != hipSuccess)
          rc = ntru_fail(NTRU_ERR_HIP, "hipMemcpyAsync (device to host) failed");
      }
      // (recorded even after a failure: whatever was enqueued for this set must be waited for before the set is reused)
      if (hipEventRecord(sl.down_done, s_down) == hipSuccess) sl.busy = true;
      else if (rc == NTRU_OK) rc = ntru_fail(NTRU_ERR_HIP, "hipEventRecord failed");
    }
    // results of the chunks still in flight, oldest first; on failure still wait so nothing is left in flight
    const std::string err = rc ? std::string(ntru_last_error()) : std::string();
    for (int t = 0; t < NTRU_HOST_SLOTS; t++) {
      const int s = (int)((k + t) % NTRU_HOST_SLOTS);
      if (rc) {
        HostSlot &sl = eng->slot[s];
        if (sl.busy) { (void)hipStreamSynchronize(eng->st_up); (void)hipStreamSynchronize(eng->st_comp); (void)hipStreamSynchronize(eng->st_down); sl.busy = false; }
        pending[s].clear();
      } else rc = drain(s);
    }
    if (!err.empty()) ntru_fail(rc, err);
    return rc;
  }
};

#endif
