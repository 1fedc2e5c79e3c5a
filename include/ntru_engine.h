/*
 * ntru_engine.h -- C ABI of the MI355X NTRU polynomial-ring engine.
 *
 * This is the drop-in boundary for the hot path of numtel/ntru-circom (reference file index.js):
 * the linear product (multiplyPolynomials, index.js:319-355), the quotient/remainder split by
 * I = 1 - x^N (dividePolynomials with b = I, index.js:358-401), the coefficient-wise reductions
 * (addPolynomials index.js:235-244, centred lift index.js:117) and the three scheme methods built
 * from them (encryptBits :87-110, decryptBits :111-140, verifyKeysInputs :141-197).
 *
 * The reference has no FFI of its own (it is a single ES module); the bindings a maintainer adds
 * are shown in INTEGRATION.md (N-API addon in ntru-circom_amd/js/, ctypes in ntru-circom_amd/engine.py).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, caller-owned buffers, nothing allocated across the ABI.
 *   - every batch array is row-major [B][N] with a fixed stride of N elements, zero padded: row b holds
 *     the N coefficients of item b.  The reference's witness arrays of length N+1 always end in 0
 *     (index.js:101-102,127-130,174-175): that element and the trimming of `value`
 *     (trimPolynomial, index.js:218-221) are added by the host-side shim, not stored on the device.
 *   - mod-q coefficients are uint16_t (q a power of two, 2 <= q <= 65536); ternary / mod-p coefficients
 *     are uint8_t; signed ternary key material f, g is int8_t in {-1, 0, 1}.
 *   - every function returns 0 on success or one of the NTRU_ERR_* codes; ntru_last_error() then
 *     returns a message for the calling thread.
 *   - *_dev entry points take DEVICE pointers and enqueue work on the engine's stream without
 *     synchronising; the same names without _dev take HOST pointers and return when the results are in
 *     the caller's buffers: the batch is cut into chunks that flow through two engine-owned streams
 *     (H2D, kernel and D2H of neighbouring chunks overlap), through pinned staging arenas that only grow
 *     -- or with no staging at all for buffers from ntru_host_alloc.  An engine is used by one thread at a time.
 *   - there is no CPU fallback: without a usable HIP device ntru_engine_create fails.
 *   - symbol preconditions (what the reference itself always produces): r in {0,1,2}; f, g in {-1,0,1}; fp and the
 *     plaintext-side values below p.  The fast kernels rely on them (the ternary add path steps over these operands by
 *     symbol class, the matrix-core path carries them as int8 digits: r <= 3, |f| <= 1); any other value is a caller
 *     error with unspecified results.  ntru_engine_set_kernel_path(1) selects the multiply-accumulate kernels, which
 *     accept arbitrary operand values for r and h, e, fq.
 *   - shared-key encrypt / decrypt with 64 <= N <= 1024 and q <= 8192 run on the int8 matrix cores (batch x Toeplitz
 *     matrix of the key, exact), and so does verify_keys with 128 <= N <= 1024, q <= 8192, p == 3 (each per-item product
 *     as a 32-row matrix product per tile distance), polymul_split with a power-of-two modulus <= 8192, the public key
 *     and the Newton rounds of the key inversion in the same N range; everything else on the vector-ALU kernel families.
 *     Pointers may have any alignment.
 */
#ifndef NTRU_ENGINE_H
#define NTRU_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTRU_OK 0
#define NTRU_ERR_NO_DEVICE 1   /* no HIP device / device id out of range */
#define NTRU_ERR_ARG 2         /* NULL pointer, negative size, ...       */
#define NTRU_ERR_UNSUPPORTED 3 /* parameter set outside what the kernels implement */
#define NTRU_ERR_HIP 4         /* a HIP runtime call failed               */

/* bits of the per-item flags byte written by ntru_verify_keys_batch: set when the reference's
 * verifyKeysInputs would throw 'invalid fq' / 'invalid fp' / 'invalid h' (index.js:159-166). */
#define NTRU_FLAG_INVALID_FQ 1
#define NTRU_FLAG_INVALID_FP 2
#define NTRU_FLAG_INVALID_H 4
/* bits of the per-key flags byte written by ntru_invert_key_batch */
#define NTRU_FLAG_NOT_UNIT_MOD2 8  /* f has no inverse modulo 2 (hence none modulo q): fq is zero */
#define NTRU_FLAG_NOT_UNIT_MODP 16 /* f has no inverse modulo p: fp is zero */

typedef struct ntru_engine ntru_engine_t;

/* Number of HIP devices visible to the process (0 if none / runtime unusable). */
int ntru_engine_device_count(void);

/* Create an engine bound to HIP device `device`.  Work is enqueued on the NULL stream until
 * ntru_engine_set_stream is called. */
int ntru_engine_create(int device, ntru_engine_t **out);
void ntru_engine_destroy(ntru_engine_t *eng);

/* Use `hip_stream` (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream) for all later calls.
 * The engine never owns the stream. */
int ntru_engine_set_stream(ntru_engine_t *eng, void *hip_stream);
/* Tuning / test knob: 0 = pick the fastest applicable kernel family (default), 1 = always the packed-u16 MAC
 * kernels, 2 = the ternary add path wherever it applies, 3 = the add path without its dot8 product, 4 = the int8
 * matrix-core path wherever it applies (encrypt / decrypt: shared key, q <= 8192, N <= 1024; verify_keys: q <= 8192,
 * p == 3, 64 <= N <= 1024), even for small N, as two independent four-wave workgroups per CU (k_encrypt_m, k_decrypt_m),
 * 5 = the matrix-core path as auto-selection runs it at large N, for every N: decrypt as ONE workgroup of two four-wave groups
 * whose matrix-loop and epilogue phases are interleaved by barriers (k_decrypt_m8; k_decrypt_m where 160 KB of LDS do not hold
 * two groups), encrypt with direct-to-LDS operand loads (k_encrypt_md; k_encrypt_m for rows that do not fit one such
 * instruction).  0 picks k_encrypt_md and, for N > 512 with every witness array, k_decrypt_m8.  Results are identical on every
 * path.  Any other value is refused (NTRU_ERR_ARG).
 * Streams: the *_dev calls that need temporaries (key inversion, the generic family) share one engine-owned scratch buffer.
 * Calls on one stream are ordered by the stream; after ntru_engine_set_stream a call first makes the new stream wait (on the
 * device) for the previous stream's use of that buffer.  The buffer only grows, and growing it frees the old one with hipFree,
 * which waits for the whole device. */
int ntru_engine_set_kernel_path(ntru_engine_t *eng, int path);
/* Name of the kernel the last *_dev call on this engine launched, e.g. "k_decrypt_s<13,13>" (for reports). */
const char *ntru_engine_last_kernel(ntru_engine_t *eng);
/* Block until everything enqueued on the engine's stream has finished. */
int ntru_engine_synchronize(ntru_engine_t *eng);

/* Message describing the last error on this thread ("" if none). */
const char *ntru_last_error(void);

/* ---- device-resident use from a host language without HIP of its own (the N-API addon) --------------------------------------
 * ntru_pipeline_batch chains generateCustomArray (index.js:461-488: the r of encryptBits, drawn on the device from a ChaCha20
 * stream) -> encryptBits (index.js:87-110) -> decryptBits (index.js:111-140) -> packOutput (index.js:572-596) for a batch of HOST
 * plaintexts m [B][N]; the intermediates stay on the GPU, chunk by chunk through the engine's three stage streams (upload, compute, download).
 *   key != NULL: r is sampled (n1 ones, n2 entries p - 1, item b from stream position first_item + b); else r [B][N] is read.
 *   f, fp both NULL: encrypt only.
 *   outputs, each optional (at least one): r_out [B][N] (the sampled r, to replay), e [B][N], value [B][N] (needs f, fp),
 *   packed [B][output_size][4] = packOutput(max, N, .) of the LAST stage's result: value with max = p - 1 when decrypting (then it
 *   comes out of the decrypt kernel itself: ntru_decrypt_pack_batch_dev), else e with max = q - 1 (out of the encrypt kernel itself when
 *   e is not asked for as well: ntru_encrypt_pack_batch_dev; sizes from ntru_pack_params). */
int ntru_pipeline_batch(ntru_engine_t *eng, int N, int q, int p, const uint16_t *h, const int8_t *f, const uint8_t *fp,
                        const uint32_t *key, uint64_t first_item, int n1, int n2, const uint8_t *r, const uint8_t *m, int64_t B,
                        uint8_t *r_out, uint16_t *e, uint8_t *value, uint64_t *packed);
/* Plain device buffers on the engine's device for use with the *_dev entry points.  ntru_dev_upload returns when `src` may be
 * reused and orders the data before every later call on the engine's stream; ntru_dev_download first waits for that stream. */
int ntru_dev_alloc(ntru_engine_t *eng, size_t bytes, void **d_ptr);
int ntru_dev_free(ntru_engine_t *eng, void *d_ptr);
int ntru_dev_upload(ntru_engine_t *eng, void *d_dst, const void *src, size_t bytes);
int ntru_dev_download(ntru_engine_t *eng, void *dst, const void *d_src, size_t bytes);

/* 1 if (N, mod) is a parameter set the kernels implement: mod a power of two <= 65536, or a small
 * modulus with N*(mod-1)^2 < 65536 (p = 3 for every NTRU set); 2 <= N <= NTRU_MAX_N. */
int ntru_engine_supports(int N, int mod);
#define NTRU_MAX_N 1920

/* ---- generic product + split: replaces multiplyPolynomials(a,b,mod) followed by
 *      dividePolynomials(.,I,mod) (index.js:319-355, 358-401) for per-item operands.
 *      a, b: [B][N] values (any uint16, reduced or not when mod is a power of two; < mod otherwise).
 *      quot[b][k] = (mod - c[N+k]) % mod,  rem[b][k] = (c[k] + c[N+k]) % mod,  c = linear product. */
int ntru_polymul_split(ntru_engine_t *eng, int N, int mod, const uint16_t *a, const uint16_t *b,
                       int64_t B, uint16_t *quot, uint16_t *rem);
int ntru_polymul_split_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_a, const uint16_t *d_b,
                           int64_t B, uint16_t *d_quot, uint16_t *d_rem);

/* ---- product of a batch with ONE shared polynomial + split: multiplyPolynomials(row, s, mod) followed by dividePolynomials(., I, mod)
 *      (index.js:319-355, 358-401) with s fixed over the batch -- e * c mod (x^N - 1) for a public polynomial c (the homomorphic
 *      plaintext-polynomial product; c = x^k rotates), or s * e for a key that is not ternary.  s: [N]; rows: [B][N] dense; quot, rem:
 *      [B][N]; quot may be NULL, like quotE.  Row b of quot / rem is byte for byte what ntru_polymul_split(a = rows, b = s repeated B
 *      times) returns: quot[b][k] = (mod - c[N+k]) % mod, rem[b][k] = (c[k] + c[N+k]) % mod, c = the linear product rows[b] * s.
 *      Domain: that of ntru_polymul_split, ntru_engine_supports(N, mod); operands are any uint16, reduced or not, when mod is a power of
 *      two, and below mod otherwise; pointers of any 2-byte alignment; B == 0 launches nothing.  Refused, each with a message of its
 *      own, before the engine is looked at and before anything is launched: B < 0; an unsupported (N, mod) (NTRU_ERR_UNSUPPORTED); a
 *      NULL s, rows or rem with B > 0; an output range that overlaps an input range or the other output; a NULL engine with valid
 *      arguments is then the usual "engine is NULL".
 *      A power-of-two mod <= 8192 with N <= 1024 on kernel paths 0 (N >= 64), 4 and 5 runs as batch x Toeplitz matrix of s on the int8
 *      matrix cores (k_mul_shared_m: rows and s both split at 128, three plane products per contraction step, exact).  Everything else
 *      -- mod > 8192, a modulus that is no power of two, N > 1024, kernel paths 1-3 -- replicates s into the engine-owned scratch and
 *      runs the per-item kernels of ntru_polymul_split_dev, in passes of at most 65536 rows: correct, not fast.
 *   _dev: enqueues on the engine's stream, does not synchronise, allocates nothing per call.
 *   host form: the rows run through the chunked pipeline; s goes up with every chunk, as h does for ntru_encrypt_batch.
 *   On ciphertexts the product multiplies the noise by the 1-norm of c ("Multiplying by a shared polynomial"). */
int ntru_mul_shared_batch(ntru_engine_t *eng, int N, int mod, const uint16_t *s, const uint16_t *rows, int64_t B, uint16_t *quot,
                          uint16_t *rem);
int ntru_mul_shared_batch_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_s, const uint16_t *d_rows, int64_t B,
                              uint16_t *d_quot, uint16_t *d_rem);

/* ---- stand-alone split: dividePolynomials(a, I, mod) (index.js:358-401 with b = I = 1 - x^N) for dividends that
 *      are already reduced into [0,mod).  a: [B][2N] (row b = the dividend's coefficients 0..2N-1, zero padded).
 *      quot[b][k] = (mod - a[N+k]) % mod, rem[b][k] = (a[k] + a[N+k]) % mod   (SURVEY.md 0.3). */
int ntru_split_by_I(ntru_engine_t *eng, int N, int mod, const uint16_t *a, int64_t B, uint16_t *quot, uint16_t *rem);
int ntru_split_by_I_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_a, int64_t B, uint16_t *d_quot,
                        uint16_t *d_rem);

/* ---- coefficient-wise sum: addPolynomials(a, b, mod) (index.js:235-244) on [B][N] rows, e.g. the additive
 *      homomorphism on ciphertexts of test/reference.test.js:46-61.  out[b][k] = (a[b][k] + b[b][k]) % mod. */
int ntru_add_batch(ntru_engine_t *eng, int N, int mod, const uint16_t *a, const uint16_t *b, int64_t B, uint16_t *out);
int ntru_add_batch_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_a, const uint16_t *d_b, int64_t B,
                       uint16_t *d_out);

/* ---- sums of ciphertexts in groups, with weights: the additive homomorphism folded over a whole tally -- addPolynomials
 *      (index.js:235-244) over every row of a group, each row first scaled as multiplyPolynomialsByScalar does -- in one pass over
 *      the rows.  rows: the dense [B][N] ciphertext array, entries below mod; weights: [B], one uint16_t < mod per row, or NULL for
 *      all ones (that path does not multiply); out: [G][N],
 *        out[g][k] = (sum over the rows of group g of weights[row] * rows[row][k]) % mod.
 *      offsets == NULL: uniform groups, group g is rows [g K, (g + 1) K), K >= 1, B = G K.  offsets != NULL: [G + 1] row indices,
 *      non-decreasing, offsets[0] >= 0; group g is rows [offsets[g], offsets[g + 1]) and K is ignored.  An empty group gives a zero row.
 *      Domain: 2 <= N <= NTRU_MAX_N, 2 <= mod <= 65536, a power of two or not; exact for groups of up to 2^31 rows (a power-of-two
 *      modulus accumulates in wrapping 32-bit words, any other in 64-bit words).  G == 0 launches nothing.
 *      Integer sums do not depend on the order of the summands: the result is the same bytes whatever the decomposition into
 *      workgroups, the grid, the chunking of the host form or the kernel path.
 *   _dev: d_offsets is a DEVICE array that the call neither reads on the host nor waits for: it does not synchronise, and the kernels
 *      (k_sum_groups, k_sum_groups_finish) cope with any distribution of group sizes.  Malformed device offsets are the caller's error
 *      (unspecified rows are read).  Groups that are split over wavefronts leave partial rows in the engine-owned scratch buffer, whose
 *      size depends on N and the grid only; nothing is allocated per call.
 *   host form: validates the offsets and weights (NTRU_ERR_ARG before any launch); the rows run through the chunked pipeline, a group
 *      larger than a chunk is accumulated across chunks on the device. */
int ntru_sum_groups(ntru_engine_t *eng, int N, int mod, const uint16_t *rows, const uint16_t *weights, const int64_t *offsets,
                    int64_t K, int64_t G, uint16_t *out);
int ntru_sum_groups_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_rows, const uint16_t *d_weights,
                        const int64_t *d_offsets, int64_t K, int64_t G, uint16_t *d_out);
/* The tally: sum = ntru_sum_groups(rows) modulo q, then decryptBits (index.js:111-140) of every sum under one private key with the
 * kernels ntru_decrypt_batch_dev picks.  sum [G][N] is needed as the intermediate (NULL is NTRU_ERR_ARG) and may be read afterwards;
 * quot1 / rem1 / quot2 may be NULL.  Row g of value, quot1, rem1, quot2 is bit-identical to ntru_decrypt_batch on sum[g]; with f, fp
 * and sum[g] it is a VerifyDecrypt witness for the tally.  Domain: that of ntru_decrypt_batch (q a power of two).  Whether value equals
 * the sum of the plaintexts modulo p depends on the noise of the summed ciphertext, as in the reference ("Tallies"). */
int ntru_tally_decrypt_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp, const uint16_t *rows,
                             const uint16_t *weights, const int64_t *offsets, int64_t K, int64_t G, uint16_t *sum, uint8_t *value,
                             uint16_t *quot1, uint16_t *rem1, uint8_t *quot2);
int ntru_tally_decrypt_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                 const uint16_t *d_rows, const uint16_t *d_weights, const int64_t *d_offsets, int64_t K, int64_t G,
                                 uint16_t *d_sum, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1, uint8_t *d_quot2);

/* ---- combining ciphertexts by a weight matrix: G linear combinations of the SAME B rows in one pass over them (one ballot counted in
 *      several totals, rows scored against several public weight vectors) -- addPolynomials (index.js:235-244) over rows scaled as
 *      multiplyPolynomialsByScalar does, once per output.  rows: [B][N], entries below mod, as for ntru_sum_groups; weights: [B][G]
 *      row-major, row b holds the G weights of ciphertext b, each below mod (the [B] weights of ntru_sum_groups widened to G columns);
 *      out: [G][N],
 *        out[g][k] = (sum over b of weights[b][g] * rows[b][k]) % mod,
 *      and row g of out is byte for byte what ntru_sum_groups(rows, column g of weights, K = B, G = 1) returns.
 *      Domain: 2 <= N <= NTRU_MAX_N; 2 <= mod <= 65536, a power of two or not; 1 <= G <= NTRU_COMBINE_MAX_G; 0 <= B <= 2^31 (B == 0
 *      writes G zero rows); pointers of any 2-byte alignment.  NTRU_ERR_ARG, each with a message of its own, before the engine is looked
 *      at and before anything is launched: anything outside the domain, a NULL buffer with B > 0 (out: always), an out range that
 *      overlaps rows or weights; a NULL engine with valid arguments is then the usual "engine is NULL".
 *      The product is one integer matrix product modulo mod, out = W^T . rows.  A power-of-two modulus on kernel paths 0, 4 and 5 runs
 *      on the int8 matrix cores (k_combine_m: two balanced digit planes per operand, wrapping int32 accumulators, exact); any other
 *      modulus, and every modulus on kernel paths 1-3, runs on the vector ALU (k_combine_v).  The rows are cut into row blocks that
 *      leave int32 partial results in the engine-owned scratch (at most 256 MiB, bounded by N, G and the grid, not by B) and
 *      k_combine_finish adds them in a fixed order.  Integer sums do not depend on the order of the summands: the bytes of out do not
 *      depend on the grid, the number of row blocks, the chunking of the host form or the kernel path.
 *   _dev: enqueues on the engine's stream, does not synchronise, allocates nothing per call; weights >= mod are the caller's error.
 *   host form: refuses a weight >= mod (NTRU_ERR_ARG naming row and column); rows and weights run through the chunked pipeline side by
 *      side, out is accumulated across chunks on the device and comes down once.
 *   Whether a combination decrypts to the weighted sum of the plaintexts depends on its noise: a weight multiplies its row's noise
 *   ("Combining ciphertexts"). */
#define NTRU_COMBINE_MAX_G 4096
int ntru_combine_batch(ntru_engine_t *eng, int N, int mod, const uint16_t *rows, const uint16_t *weights, int64_t B, int G,
                       uint16_t *out);
int ntru_combine_batch_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_rows, const uint16_t *d_weights, int64_t B, int G,
                           uint16_t *d_out);

/* ---- packed ciphertexts: the three calls above and decryptBits on ciphertexts that arrive in the circuits' wire format,
 *      packOutput(mod - 1, N, e) (index.js:572-596) -- what CombineArray makes public and what ntru_encrypt_pack_batch_dev,
 *      ntru_pipeline_batch(packed) and ntru_keygen_batch(packed_h) emit -- without unpacking them first.
 *      packed: [B][output_size][4] uint64_t with (bits, per, arr_len, output_size) = ntru_pack_params(mod - 1, N, ...): a row is
 *      output_size field elements of four little-endian limbs, coefficient i is the bits-wide field at bit (i % per) * bits of element
 *      i / per (fields may straddle limbs).  Fields with index >= N and the bits of an element above per * bits are IGNORED, whatever
 *      they hold, as unpackInput's mask (index.js:598-620) ignores them.  Any 8-byte aligned address will do.
 *   ntru_sum_groups_packed   ntru_sum_groups on the unpacked rows: the same arguments, groups, weights, domain, exactness and checks, and
 *                          the same bytes in out, dense [G][N] (a raw field is below 2^bits <= 65536, so the sums are exact for fields that
 *                          are not below mod as well).  One kernel reads the packed rows once, 32 output_size bytes per row
 *                          (k_sum_groups_packed; groups that are split over wavefronts are completed by k_sum_groups_finish).
 *                          _dev: d_offsets is a DEVICE array that is neither read on the host nor waited for; no synchronisation;
 *                          scratch bounded by N and the grid; nothing allocated per call.  G == 0 launches nothing.
 *                          host form: validates offsets and weights (NTRU_ERR_ARG before any launch), streams the packed rows through the
 *                          chunked pipeline and accumulates a group larger than a chunk across chunks.
 *   ntru_tally_decrypt_packed_batch   ntru_tally_decrypt_batch with packed rows: ntru_sum_groups_packed modulo q into sum (dense [G][N],
 *                          needed as the intermediate), then the decrypt of ntru_tally_decrypt_batch.
 *   ntru_decrypt_packed_batch   ntru_decrypt_batch of the unpacked rows: row b of value, quot1, rem1, quot2 (the last three may be NULL)
 *                          is bit-identical to ntru_decrypt_batch on unpacked row b.  The rows are unpacked (k_unpack_rows) into the
 *                          engine-owned scratch buffer in passes of at most 65536 rows and decrypted by the kernels ntru_decrypt_batch_dev
 *                          picks; the _dev form does not synchronise and allocates nothing per call. */
int ntru_sum_groups_packed(ntru_engine_t *eng, int N, int mod, const uint64_t *packed, const uint16_t *weights,
                           const int64_t *offsets, int64_t K, int64_t G, uint16_t *out);
int ntru_sum_groups_packed_dev(ntru_engine_t *eng, int N, int mod, const uint64_t *d_packed, const uint16_t *d_weights,
                               const int64_t *d_offsets, int64_t K, int64_t G, uint16_t *d_out);
int ntru_tally_decrypt_packed_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp,
                                    const uint64_t *packed, const uint16_t *weights, const int64_t *offsets, int64_t K, int64_t G,
                                    uint16_t *sum, uint8_t *value, uint16_t *quot1, uint16_t *rem1, uint8_t *quot2);
int ntru_tally_decrypt_packed_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                        const uint64_t *d_packed, const uint16_t *d_weights, const int64_t *d_offsets, int64_t K,
                                        int64_t G, uint16_t *d_sum, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1,
                                        uint8_t *d_quot2);
int ntru_decrypt_packed_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp, const uint64_t *packed,
                              int64_t B, uint8_t *value, uint16_t *quot1, uint16_t *rem1, uint8_t *quot2);
int ntru_decrypt_packed_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                  const uint64_t *d_packed, int64_t B, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1,
                                  uint8_t *d_quot2);

/* ---- measuring noise: how much room a ciphertext row has left under a private key.  For a row e ([N], reduced modulo q, q a power of
 *      two) and a key f ([N], symbols in {-1, 0, 1}: the precondition of ntru_decrypt_batch),
 *        a_k      = (f * e mod x^N - 1)_k mod q       byte for byte the rem1 that ntru_decrypt_batch returns for that row and key
 *        c_k      = a_k > q/2 ? a_k - q : a_k         the threshold of both lift modes; it is strict: a_k = q/2 stays +q/2
 *        peak     = max_k |c_k|                       in [0, q/2]: a uint16_t (32768 at most, at q = 65536)
 *        energy   = sum_k c_k^2                       a uint64_t (below 2^41 for every N and q of the domain)
 *      Neither depends on p, on fp or on the lift mode (ntru_engine_set_lift changes nothing here).
 *      What the numbers mean: with A = p r*g + f*m taken over the integers, decryption under the centred lift is right exactly when
 *      every A_k lies in (-q/2, q/2].  Then c = A, peak is the true infinity norm of A and q/2 - peak is the room left.  Once some A_k
 *      has left that interval a has wrapped and peak is only the norm of the wrapped value: a wrapped row cannot be told from a merely
 *      noisy one with certainty, which is why callers keep a guard band.  Growth: sums add A (ntru_sum_groups, the tallies), weights
 *      and a polynomial c scale it (ntru_combine_batch: by the weight; ntru_mul_shared_batch: by at most the 1-norm of c), and every
 *      mix round adds a fresh p r*g (ntru_reencrypt_batch, ntru_mix_batch).  INTEGRATION.md, "Measuring noise".
 *      f: [N]; e: [B][N] dense; packed: [B][output_size][4] in the wire format of "packed ciphertexts" above (ignored fields and bits
 *      as there); peak: [B]; energy: [B].  Either output may be NULL, but not both.  energy needs 8-byte alignment; e and peak take any
 *      2-byte alignment, packed any 8-byte alignment.  Domain: 2 <= N <= NTRU_MAX_N, q a power of two with 2 <= q <= 65536, B >= 0;
 *      B == 0 launches nothing.  Refused, each with a message of its own, before the engine is looked at and before anything is
 *      launched (NTRU_ERR_UNSUPPORTED for the domain, NTRU_ERR_ARG otherwise): B < 0; (N, q) outside the domain; a NULL f or NULL rows
 *      with B > 0; both outputs NULL; a misaligned energy; an output range that overlaps an input range or the other output.  A NULL
 *      engine with valid arguments is then the usual "engine is NULL".
 *      Wherever the shared-key decrypt runs on the matrix cores (q <= 8192, N <= 1024, kernel paths 0 with N >= 64, 4 and 5) one
 *      kernel, k_noise_m, runs decrypt's first product and reduces it in its epilogue: one of decrypt's two products, 10 bytes stored
 *      per row.  Everything else runs the vector-ALU decrypt for its rem1 into the engine-owned scratch, in passes of at most 65536
 *      rows, and reduces the pass (k_noise_rows); ntru_engine_last_kernel then reports noise_rows(<the product's kernel>).  The packed
 *      forms unpack a pass into scratch first.  Scratch is bounded in B.
 *   _dev: enqueues on the engine's stream, does not synchronise, allocates nothing per call.
 *   host forms: the rows run through the chunked pipeline, f goes up with every chunk; 2 and 8 bytes per row come down. */
int ntru_noise_batch(ntru_engine_t *eng, int N, int q, const int8_t *f, const uint16_t *e, int64_t B, uint16_t *peak, uint64_t *energy);
int ntru_noise_batch_dev(ntru_engine_t *eng, int N, int q, const int8_t *d_f, const uint16_t *d_e, int64_t B, uint16_t *d_peak,
                         uint64_t *d_energy);
int ntru_noise_packed_batch(ntru_engine_t *eng, int N, int q, const int8_t *f, const uint64_t *packed, int64_t B, uint16_t *peak,
                            uint64_t *energy);
int ntru_noise_packed_batch_dev(ntru_engine_t *eng, int N, int q, const int8_t *d_f, const uint64_t *d_packed, int64_t B,
                                uint16_t *d_peak, uint64_t *d_energy);

/* ---- on-device ternary sampler: generateCustomArray(N, n1, n2) (index.js:461-488) for B items, so that encryptBits'
 *      randomness r never crosses PCIe.  Row b (item index first_item + b) gets n1 ones, n2 entries equal to `other`
 *      (2 = p-1 for r after the index.js:89 map) and zeros, shuffled exactly like the reference: for i = N-1 .. 1:
 *      j = u32 % (i+1), swap -- with the u32 of step t taken from word t of the ChaCha20 keystream (RFC 8439 block
 *      function) under `key` (8 words) with nonce (item_lo, item_hi, 0x4e545255) and block counter 0,1,2,...
 *      A host replays the stream with any ChaCha20 implementation.  key is a HOST pointer in both variants. */
int ntru_sample_ternary(ntru_engine_t *eng, int N, int n1, int n2, int other, const uint32_t *key, uint64_t first_item,
                        int64_t B, uint8_t *out);
int ntru_sample_ternary_dev(ntru_engine_t *eng, int N, int n1, int n2, int other, const uint32_t *key,
                            uint64_t first_item, int64_t B, uint8_t *d_out);
/* Rounds of the sampler's block function: 20 (ChaCha20 as in RFC 8439: the default), 12 or 8 (ChaCha12 / ChaCha8: the same
 * quarter round, state and output rule, fewer double rounds).  generateCustomArray's contract (index.js:461-488) is the shuffle
 * order and its `u32 % (i + 1)` draws, not the generator behind crypto.getRandomValues; the sampler kernel is bound by the
 * vector issue of these rounds, and a host replays whichever variant it asked for.  Applies to ntru_sample_ternary[_dev] and to the
 * sampler stage of ntru_pipeline_batch of this engine until changed. */
int ntru_engine_set_sampler_rounds(ntru_engine_t *eng, int rounds);
int ntru_engine_get_sampler_rounds(ntru_engine_t *eng);

/* ---- encryptBits (index.js:87-110) for B plaintexts under one public key.
 *      h[N] in [0,q); r[B][N] in {0,1,2} (the sampler output with -1 already mapped to p-1, index.js:89);
 *      m[B][N] plaintext coefficients (README: 0/1/2; any byte is accepted and added mod q).
 *      e = remainderE (the ciphertext), quotE = quotientE (may be NULL when the witness is not wanted). */
int ntru_encrypt_batch(ntru_engine_t *eng, int N, int q, const uint16_t *h, const uint8_t *r, const uint8_t *m,
                       int64_t B, uint16_t *e, uint16_t *quotE);
int ntru_encrypt_batch_dev(ntru_engine_t *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r,
                           const uint8_t *d_m, int64_t B, uint16_t *d_e, uint16_t *d_quotE);

/* ---- decryptBits (index.js:111-140) for B ciphertexts under one private key.
 *      f[N] in {-1,0,1}; fp[N] in [0,p); e[B][N] in [0,q).
 *      value = remainder2; quot1 / rem1 / quot2 = quotient1 / remainder1 / quotient2 (each may be NULL).
 *      The centred lift is the reference's `x > q/2 ? (x+1)%p : x%p` verbatim unless the engine is in
 *      NTRU_LIFT_CENTRED (ntru_engine_set_lift below). */
int ntru_decrypt_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp,
                       const uint16_t *e, int64_t B, uint8_t *value, uint16_t *quot1, uint16_t *rem1,
                       uint8_t *quot2);
int ntru_decrypt_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                           const uint16_t *d_e, int64_t B, uint8_t *d_value, uint16_t *d_quot1,
                           uint16_t *d_rem1, uint8_t *d_quot2);
/* The lift of decryptBits, a mode of the engine.  The reference maps a = f e mod q into mod p with `x > q/2 ? (x+1)%p : x%p`
 * (index.js:117).  The representative of x > q/2 is x - q, so the `+ 1` is right only when -q = 1 (mod p): for p = 3 at q = 128,
 * 2048, 8192, not at q = 256, 1024, 4096, 16384, 65536, and for hardly any q once p is 5 or 7.  Where it is wrong, decryptBits does
 * not return the plaintext ("The lift").
 *   NTRU_LIFT_REFERENCE   index.js:117 verbatim (the default of a new engine): bit-identical to the reference, and what the
 *                         VerifyDecrypt circuit (which hard-codes `+ gt`) accepts as a witness.
 *   NTRU_LIFT_CENTRED     x > q/2 ? (x - q) mod p : x % p, i.e. the addend (p - q % p) % p in place of 1.  quot1 / rem1 are what they
 *                         were; value and quot2 come from the centred b.  Where the addend is 1 both modes give the same bytes.
 * The threshold is strict in both modes (x = q/2 is lifted as positive).  The same kernels run in both modes: the addend is one
 * kernel argument.  Honoured by everything that runs decryptBits: ntru_decrypt_batch[_dev], ntru_decrypt_batch_pitched_dev,
 * ntru_decrypt_pack_batch_dev, ntru_decrypt_peritem_batch[_dev], ntru_decrypt_bytes_batch[_dev], ntru_tally_decrypt_batch[_dev],
 * ntru_tally_decrypt_packed_batch[_dev], ntru_decrypt_packed_batch[_dev], the decrypt stage of ntru_pipeline_batch and
 * ntru_pipeline_bytes_batch, ntru_scan_bytes_batch[_dev], ntru_scan_bytes_packed_batch[_dev], ntru_count_bytes_batch[_dev],
 * ntru_count_bytes_packed_batch[_dev], ntru_multi_decrypt_batch (ntru_multi_set_lift). ntru_check_decrypt_batch checks the circuit and
 * ntru_verify_keys_batch has no lift: neither changes.
 * The mode is read when a call enqueues and reaches the kernel by value: a _dev call enqueued before a later ntru_engine_set_lift
 * keeps the mode it was enqueued with.  As with ntru_engine_set_stream and ntru_engine_set_kernel_path, do not change it while a
 * host-form call on that engine is running.
 * ntru_engine_set_lift: a NULL engine, then an unknown mode, is NTRU_ERR_ARG.  ntru_engine_get_lift(NULL) is NTRU_LIFT_REFERENCE. */
#define NTRU_LIFT_REFERENCE 0
#define NTRU_LIFT_CENTRED 1
int ntru_engine_set_lift(ntru_engine_t *eng, int lift);
int ntru_engine_get_lift(ntru_engine_t *eng);

/* ---- byte messages as packed bits: encryptStr / decryptStr (index.js:80-86) and the stringToBits / bitsToString under them
 *      (index.js:538-556) on the device, for messages of any length and with one BIT per plaintext bit across the bus.
 *      A message block is nbytes whole bytes, 1 <= nbytes <= N / 8 (integer division), 8 <= N <= NTRU_MAX_N; the caller cuts a longer
 *      message into blocks (the reference cannot: "Max N bits since there's no provision to split into words", index.js:81).
 *      Bit order is stringToBits' (index.js:542): coefficient 8 i + j of row b is (bytes[b][i] >> (7 - j)) & 1, most significant bit
 *      first; the coefficients 8 nbytes .. N - 1 are the pad.  Byte arrays are dense [B][nbytes], coefficient rows dense [B][N]
 *      uint8_t, flags [B]; pointers may have any alignment.  Anything outside the domain is NTRU_ERR_ARG before any launch; B == 0
 *      launches nothing.
 *   ntru_bytes_to_rows     stringToBits (index.js:538-546) of every block, the pad written as 0: every byte of m is defined.
 *   ntru_rows_to_bytes     bitsToString (index.js:548-556) of every row for value in {0, 1}: bit = value & 1.  flags[b] (flags may be
 *                          NULL) is 0 or the OR of the two bits below -- what the reference can only show as a garbled string
 *                          (test/reference.test.js:15-25, :46-61): a wrong key, a decryption failure, a sum of plaintexts.
 *   ntru_encrypt_bytes_batch   = ntru_encrypt_batch (index.js:87-110) on the rows of ntru_bytes_to_rows: encryptStr (index.js:80-83) per
 *                          block with r given; bit-identical e and quotE (quotE may be NULL).
 *   ntru_decrypt_bytes_batch   = value-only ntru_decrypt_batch (index.js:111-140), then ntru_rows_to_bytes: decryptStr (index.js:84-86)
 *                          per block, without its trimming (the caller's length frames the message).
 *   The _dev forms do not synchronise and allocate nothing per call: the intermediate rows (m, value) live in the engine-owned scratch
 *   buffer, in passes of at most 65536 rows, so its size is bounded in B.  The host forms run the chunked pipeline.
 *   Kernels: k_bytes_to_rows, k_rows_to_bytes (message_bytes.hip); the scheme kernels are the ones ntru_encrypt_batch_dev /
 *   ntru_decrypt_batch_dev pick. */
#define NTRU_FLAG_NOT_BITS 32    /* some coefficient k < 8 nbytes of the row is above 1 */
#define NTRU_FLAG_PAD_NONZERO 64 /* some coefficient 8 nbytes <= k < N of the row is not 0 */
int ntru_bytes_to_rows(ntru_engine_t *eng, int N, int nbytes, const uint8_t *bytes, int64_t B, uint8_t *m);
int ntru_bytes_to_rows_dev(ntru_engine_t *eng, int N, int nbytes, const uint8_t *d_bytes, int64_t B, uint8_t *d_m);
int ntru_rows_to_bytes(ntru_engine_t *eng, int N, int nbytes, const uint8_t *value, int64_t B, uint8_t *bytes, uint8_t *flags);
int ntru_rows_to_bytes_dev(ntru_engine_t *eng, int N, int nbytes, const uint8_t *d_value, int64_t B, uint8_t *d_bytes,
                           uint8_t *d_flags);
int ntru_encrypt_bytes_batch(ntru_engine_t *eng, int N, int q, int nbytes, const uint16_t *h, const uint8_t *r, const uint8_t *bytes,
                             int64_t B, uint16_t *e, uint16_t *quotE);
int ntru_encrypt_bytes_batch_dev(ntru_engine_t *eng, int N, int q, int nbytes, const uint16_t *d_h, const uint8_t *d_r,
                                 const uint8_t *d_bytes, int64_t B, uint16_t *d_e, uint16_t *d_quotE);
int ntru_decrypt_bytes_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *f, const uint8_t *fp,
                             const uint16_t *e, int64_t B, uint8_t *bytes, uint8_t *flags);
int ntru_decrypt_bytes_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *d_f, const uint8_t *d_fp,
                                 const uint16_t *d_e, int64_t B, uint8_t *d_bytes, uint8_t *d_flags);
/* ntru_pipeline_batch (above) with the plaintext as bytes at both ends: msg [B][nbytes] in place of m; msg_out [B][nbytes] and flags [B]
 * (what ntru_decrypt_bytes_batch returns for the fresh ciphertexts) in place of value -- both need the decrypt stage (f, fp).  m and
 * value are device-only rows of a chunk and never cross the bus.  Either a sampler key or r is given; r_out and e are optional; at
 * least one output.  Argument checks as ntru_pipeline_batch. */
int ntru_pipeline_bytes_batch(ntru_engine_t *eng, int N, int q, int p, const uint16_t *h, const int8_t *f, const uint8_t *fp,
                              const uint32_t *key, uint64_t first_item, int n1, int n2, const uint8_t *r, int nbytes,
                              const uint8_t *msg, int64_t B, uint8_t *r_out, uint16_t *e, uint8_t *msg_out, uint8_t *flags);

/* ---- scanning: which rows of a batch does a key decrypt to a well-formed message that carries the expected padding?  The read side of
 *      the README's "pad the message with data that can be confirmed during decryption": decryptStr (index.js:84-86) on decryptBits
 *      (index.js:111-140) for every row under each of K private keys, tested and compacted on the device, so that the hits alone cross
 *      the bus.
 *      Row b is a HIT for key k when, for value = decryptBits(e[b]).value under (f[k], fp[k]):
 *        - ntru_rows_to_bytes(value) gives flag byte 0: the first 8 nbytes coefficients are 0 or 1 and every later one is 0;
 *        - the bytes [tag_off, tag_off + tag_len) of the message it gives equal tag[0 .. tag_len).
 *      tag is a HOST pointer in every form, read when the call is made and handed to the kernels by value; 0 <= tag_len <=
 *      NTRU_SCAN_MAX_TAG, tag_off >= 0, tag_off + tag_len <= nbytes; tag_len == 0 tests the flags only (tag may then be NULL).
 *      f [K][N] int8_t, fp [K][N] uint8_t, K >= 1; e [B][N] uint16_t, or packed [B][output_size][4] uint64_t, the wire format of
 *      "packed ciphertexts" above (ignored fields and bits as there).
 *      count [K] int64_t: count[k] is SET to the number of hits of key k among the B rows; it may exceed max_hits.
 *      hit_row [K][max_hits] int64_t, hit_bytes [K][max_hits][nbytes]: the first min(count[k], max_hits) hits of key k in ascending
 *      row order -- the row index, and the nbytes message bytes as ntru_rows_to_bytes writes them.  Nothing behind that prefix is
 *      written.  max_hits == 0 only counts (the hit buffers may be NULL).  hit_row needs 8-byte alignment, hit_bytes none.
 *      The result is the same bytes whatever the launch shape, the pass size, the chunking of the host form and the kernel path:
 *      positions come from prefix sums, never from the arrival order of an atomic.
 *      Domain: that of ntru_decrypt_bytes_batch; the packed forms as ntru_decrypt_packed_batch.  A NULL buffer, K < 1, a tag outside
 *      the message, max_hits < 0 are NTRU_ERR_ARG before anything is launched; B == 0 sets the counts to 0.  The lift is the
 *      engine's mode (ntru_engine_set_lift), read at enqueue.
 *   _dev forms: enqueue on the engine's stream, do not synchronise and allocate nothing per call beyond the engine-owned scratch
 *      buffer: rows go in passes of at most 65536; per pass (packed: k_unpack_rows first) and key, ntru_decrypt_batch_dev and
 *      ntru_rows_to_bytes_dev run as they are into scratch, then k_scan_mark (one hit count per 256 rows), k_scan_offsets (one
 *      workgroup: exclusive offsets + the key's running count d_count[k]) and k_scan_emit (scan_hits.hip).
 *   host forms: the rows stream through the chunked pipeline with the keys as shared inputs; counts and hits stay on the device until
 *      the last chunk, then the K counts and the stored prefixes come down.  count is a host array. */
#define NTRU_SCAN_MAX_TAG 32
int ntru_scan_bytes_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, int K, const int8_t *f, const uint8_t *fp,
                          const uint16_t *e, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int64_t max_hits,
                          int64_t *hit_row, uint8_t *hit_bytes, int64_t *count);
int ntru_scan_bytes_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, int K, const int8_t *d_f, const uint8_t *d_fp,
                              const uint16_t *d_e, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int64_t max_hits,
                              int64_t *d_hit_row, uint8_t *d_hit_bytes, int64_t *d_count);
int ntru_scan_bytes_packed_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, int K, const int8_t *f, const uint8_t *fp,
                                 const uint64_t *packed, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int64_t max_hits,
                                 int64_t *hit_row, uint8_t *hit_bytes, int64_t *count);
int ntru_scan_bytes_packed_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, int K, const int8_t *d_f,
                                     const uint8_t *d_fp, const uint64_t *d_packed, int64_t B, int tag_off, int tag_len,
                                     const uint8_t *tag, int64_t max_hits, int64_t *d_hit_row, uint8_t *d_hit_bytes,
                                     int64_t *d_count);

/* ---- counting: how many rows of a batch decrypt to each choice, per group?  The end of a ballot pipeline: a homomorphic tally counts
 *      at most p - 1 votes per coefficient, so after the last mix step every row is decrypted (decryptStr, index.js:84-86, on
 *      decryptBits, index.js:111-140), the choice is read out of the message and counted.  One decrypt of the batch classifies every
 *      row on the device; only the table, and optionally one class id per row, cross the bus.
 *      For value = decryptBits(e[b]).value under (f, fp) and (bytes, flag) = ntru_rows_to_bytes(value), cls(b) is the FIRST of these
 *      that applies, with n_bins = n_choices + 3:
 *        1. flag != 0                                                          NTRU_COUNT_MALFORMED(n_choices) = n_choices + 2
 *        2. bytes [tag_off, tag_off + tag_len) differ from tag[0 .. tag_len)   NTRU_COUNT_BAD_TAG(n_choices)   = n_choices + 1
 *        3. v = the big-endian integer of bytes [field_off, field_off + field_len); v < first_choice or
 *           v - first_choice >= n_choices (compared in 64 bits: first_choice + n_choices may pass 2^32)
 *                                                                              NTRU_COUNT_OTHER(n_choices)     = n_choices
 *        4. otherwise                                                          v - first_choice
 *      tag is a HOST pointer in every form, as in "scanning": 0 <= tag_len <= NTRU_SCAN_MAX_TAG, tag_off >= 0, tag_off + tag_len <=
 *      nbytes; tag_len == 0 skips step 2 (tag may then be NULL).  1 <= field_len <= 4, field_off >= 0, field_off + field_len <= nbytes;
 *      the field may overlap the tag.  first_choice is a 32-bit value, 0 <= first_choice < 2^32 (the parameter is a uint64_t as
 *      every unsigned scalar of this header).  1 <= n_choices <= NTRU_COUNT_MAX_CHOICES, G >= 1, G * n_bins <= NTRU_COUNT_MAX_BINS.
 *      f [N] int8_t, fp [N] uint8_t: one private key.  e [B][N] uint16_t, or packed [B][output_size][4] uint64_t, the wire format of
 *      "packed ciphertexts" above (ignored fields and bits as there).  group [B] int32_t: the group of every row, or NULL -- then G
 *      must be 1 and every row is in group 0.
 *      count [G][n_bins] int64_t is SET: count[g][c] is the number of rows with group == g and cls == c.  Every row with a valid group
 *      lands in exactly one bin, so count[g] sums to the size of group g.  cls [B] int32_t (may be NULL) receives cls(b).  count
 *      needs 8-byte alignment, group and cls 4-byte alignment.
 *      A group id outside [0, G): the _dev forms count such a row nowhere and give it cls[b] = -1; the host forms reject it as
 *      NTRU_ERR_ARG before any launch and name the index (as ntru_reencrypt_batch treats src).
 *      Integer counts do not depend on the order of the adds: the bytes of count and cls are the same whatever the launch shape, the
 *      pass size, the kernel path, the route the bins are accumulated by and the chunking of the host form.
 *      Domain: that of ntru_decrypt_bytes_batch; the packed forms as ntru_decrypt_packed_batch.  Each of these is NTRU_ERR_ARG with a
 *      message of its own, before the engine is looked at: a NULL buffer, a tag or a field outside the message, first_choice, n_choices, G
 *      or G * n_bins out of range, a NULL group with G > 1, count and cls that overlap.  B == 0 sets the counts to 0 and launches nothing
 *      else.  The lift is the engine's mode (ntru_engine_set_lift), read at enqueue.
 *   _dev forms: enqueue on the engine's stream, do not synchronise and allocate nothing per call beyond the engine-owned scratch
 *      buffer: d_count is cleared on the stream, then rows go in passes of at most 65536; per pass (packed: k_unpack_rows first)
 *      ntru_decrypt_batch_dev and ntru_rows_to_bytes_dev run as they are into scratch, then k_count_classify (count_bytes.hip), one lane
 *      per row: up to 8192 bins are counted in a workgroup-private LDS histogram and flushed with one 64-bit atomic add per non-zero
 *      bin, larger tables take one 64-bit atomic add per row.
 *   host forms: the rows (and group) stream through the chunked pipeline with the key as shared inputs and cls as a per-row output;
 *      the table stays on the device until the last chunk and comes down once.  count is a host array. */
#define NTRU_COUNT_MAX_CHOICES 65536
#define NTRU_COUNT_MAX_BINS (1 << 24)
#define NTRU_COUNT_OTHER(n_choices) (n_choices)
#define NTRU_COUNT_BAD_TAG(n_choices) ((n_choices) + 1)
#define NTRU_COUNT_MALFORMED(n_choices) ((n_choices) + 2)
int ntru_count_bytes_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *f, const uint8_t *fp, const uint16_t *e,
                           int64_t B, int tag_off, int tag_len, const uint8_t *tag, int field_off, int field_len,
                           uint64_t first_choice, int n_choices, int G, const int32_t *group, int64_t *count, int32_t *cls);
int ntru_count_bytes_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *d_f, const uint8_t *d_fp,
                               const uint16_t *d_e, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int field_off,
                               int field_len, uint64_t first_choice, int n_choices, int G, const int32_t *d_group, int64_t *d_count,
                               int32_t *d_cls);
int ntru_count_bytes_packed_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *f, const uint8_t *fp,
                                  const uint64_t *packed, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int field_off,
                                  int field_len, uint64_t first_choice, int n_choices, int G, const int32_t *group, int64_t *count,
                                  int32_t *cls);
int ntru_count_bytes_packed_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *d_f, const uint8_t *d_fp,
                                      const uint64_t *d_packed, int64_t B, int tag_off, int tag_len, const uint8_t *tag,
                                      int field_off, int field_len, uint64_t first_choice, int n_choices, int G,
                                      const int32_t *d_group, int64_t *d_count, int32_t *d_cls);

/* ---- encryptBits and decryptBits with a SEPARATE key pair for every item (one ciphertext per recipient, one decryption per key
 *      holder): h, f and fp are [B][N] batch arrays with the types and layout of ntru_keygen_batch's outputs, so its device arrays
 *      feed straight in.  Row b of every result is exactly what ntru_encrypt_batch / ntru_decrypt_batch return for item b's input
 *      under item b's key: every witness array, the centred lift, the symbol preconditions, any byte of m added mod q.  The witness
 *      outputs (quotE; quot1, rem1, quot2) may be NULL.  Domain as above: 2 <= N <= NTRU_MAX_N, q a power of two <= 65536,
 *      ntru_engine_supports(N, p); anything else is NTRU_ERR_ARG / NTRU_ERR_UNSUPPORTED before any launch, B == 0 launches nothing.
 *      128 <= N <= 1024 (64 with kernel path 4), q <= 8192 (and p == 3 for decrypt) run on the int8 matrix cores, one item per
 *      wavefront (k_encrypt_pi_m, k_decrypt_pi_m); elsewhere, and on kernel paths 1-3, the call composes per-item products
 *      (ntru_polymul_split_dev) with elementwise steps, its temporaries in an engine-owned buffer that only grows.  The _dev forms
 *      do not synchronise and allocate nothing per call; the host forms run the chunked pipeline. */
int ntru_encrypt_peritem_batch(ntru_engine_t *eng, int N, int q, const uint16_t *h, const uint8_t *r, const uint8_t *m,
                               int64_t B, uint16_t *e, uint16_t *quotE);
int ntru_encrypt_peritem_batch_dev(ntru_engine_t *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r,
                                   const uint8_t *d_m, int64_t B, uint16_t *d_e, uint16_t *d_quotE);
int ntru_decrypt_peritem_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp, const uint16_t *e,
                               int64_t B, uint8_t *value, uint16_t *quot1, uint16_t *rem1, uint8_t *quot2);
int ntru_decrypt_peritem_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                   const uint16_t *d_e, int64_t B, uint8_t *d_value, uint16_t *d_quot1,
                                   uint16_t *d_rem1, uint8_t *d_quot2);

/* The same two operations on PITCHED batch arrays: row b of every batch array (r, m, e, quotE / e, value, quot1, rem1,
 * quot2) starts at element b * ld of its array, ld >= N elements (so 2 * ld bytes for the uint16 arrays and ld bytes for
 * the byte arrays); each array holds B * ld elements, the ld - N pad elements of a row are neither read into the result
 * nor written.  ld == N is the dense layout of the entry points above.  A pitch that makes rows start on cache-line
 * boundaries (ld a multiple of 64) lets the result stores go out as whole lines: at N = 821 the store pattern alone
 * reaches 3.3 TB/s at ld = 832 against 2.4 TB/s at ld = 821; inside the kernels that is worth 5-7 % of encrypt and
 * 2-3 % of a round trip (EXPERIMENTS.md round 1, profiles/archive/r01_bench_row_pitch_ab.jsonl).  The reference has no memory
 * layout of its own (JS arrays, index.js:87-140), so the pitch is purely the host binding's choice.
 * Only the matrix-core kernels take a pitch: with ld != N the call fails with NTRU_ERR_UNSUPPORTED where they do not
 * apply (kernel path 1-3 forced, q > 8192, N or ld > 1024, p != 3). */
int ntru_encrypt_batch_pitched_dev(ntru_engine_t *eng, int N, int q, int ld, const uint16_t *d_h, const uint8_t *d_r,
                                   const uint8_t *d_m, int64_t B, uint16_t *d_e, uint16_t *d_quotE);
int ntru_decrypt_batch_pitched_dev(ntru_engine_t *eng, int N, int q, int p, int ld, const int8_t *d_f,
                                   const uint8_t *d_fp, const uint16_t *d_e, int64_t B, uint8_t *d_value,
                                   uint16_t *d_quot1, uint16_t *d_rem1, uint8_t *d_quot2);

/* loadPrivateKeyF / polyInv (index.js:30-49, 491-514) for B keys: fq[b] = f[b]^-1 in Z_q[x]/(x^N - 1) (q a power of two:
 * inverse modulo 2, then Newton rounds v <- 2v - f v^2), fp[b] = f[b]^-1 modulo p = 3; f in {-1,0,1} (any other int8
 * coefficient counts by its value, in the inversions and in every Newton round alike).  The inverse is
 * unique, so for units the result equals the reference's Euclidean algorithm bit for bit.  For f that is not a unit the
 * matching flag is set and the row is zero; the reference throws 'invalid_gcd' / 'invalid fq' for most such f but its
 * `&&` checks (index.js:41-45, :451) accept some and return meaningless polynomials -- that artefact is not reproduced, and neither
 * does ntru_keygen_batch reproduce it: its redraw keeps the first f that is a unit, where the reference may keep an earlier non-unit.
 * Either of fq / fp may be NULL when only the other inverse is wanted (polyInv(f, I, 3) / polyInv(f, I, q)).
 * The Newton temporaries (4 x 2N bytes per key, at most 65536 keys at a time) live in an engine-owned buffer that only
 * grows; nothing is allocated per call and the _dev form does not synchronise.  [§8(f) #1] */
int ntru_invert_key_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, int64_t B, uint16_t *fq, uint8_t *fp,
                          uint8_t *flags);
int ntru_invert_key_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, int64_t B, uint16_t *d_fq,
                              uint8_t *d_fp, uint8_t *d_flags);

/* ---- key generation: generatePrivateKeyF + generateNewPublicKeyGH (index.js:51-79) for B items in one call, non-units redrawn on the
 *      device.  Item i = first_item + b (0 <= b < B, first_item + B <= 2^40); every position below is a stream position of
 *      ntru_sample_ternary, always with the 20-round ChaCha20 stream whatever ntru_engine_set_sampler_rounds says (the engine's setting is
 *      the same after the call):
 *        g[b]          row 0 of ntru_sample_ternary(N, dg, dg, 255, key, (1 << 40) + i, 1) as int8 (255 = -1), drawn once;
 *        attempt t     row 0 of ntru_sample_ternary(N, df, df - 1, 255, key, (t << 44) + i, 1), t = 0 .. max_tries - 1;
 *        f[b]          the first attempt that is a unit modulo 2 and modulo p; fq[b], fp[b] its inverses, bit-identical to
 *                      ntru_invert_key_batch; h[b] = ntru_public_key_batch(fq[b], g[b]); tries[b] = t + 1, flags[b] = 0;
 *        no unit       flags[b] = the NTRU_FLAG_NOT_UNIT_MOD2 / _MODP bits of the last attempt, f[b] = the last attempt, fq, fp and h
 *                      zero rows, tries[b] = max_tries.  The call still returns NTRU_OK: a failed item is data (the shims throw the
 *                      reference's 'Could not find invertible f', index.js:63).
 *      The results of item i depend on (key, i, N, q, df, dg, max_tries) only -- not on B, chunking, the device or the kernel path -- so
 *      a host replays any item with a stock ChaCha20 ("Generating keys").  Unlike the reference, whose `&&` checks
 *      (index.js:41-45) accept some non-units, every kept f is a unit (see ntru_invert_key_batch).
 *      `key` (8 words, a HOST pointer) is secret material: take it from a CSPRNG, and never use it as the key that draws the encryption
 *      randomness r -- position i of attempt 0 would be the r of item i.
 *      Domain: p == 3, q a power of two with 2 <= q and p * (q - 1) < 65536 (the public key's domain), 2 <= N <= NTRU_MAX_N, 1 <= df,
 *      2 df - 1 <= N, 0 <= dg, 2 dg <= N, 1 <= max_tries <= 255; anything else is NTRU_ERR_ARG / NTRU_ERR_UNSUPPORTED before any launch.
 *   _dev: d_work is a caller-owned device workspace of ntru_keygen_workspace_bytes(N, B) bytes (bounded in B: redraws run in passes of
 *      at most 4096 rows); nothing is allocated per call.  Every output is needed except d_tries (may be NULL).  Unlike the other _dev
 *      calls this one SYNCHRONISES the engine's stream: it reads back one 4-byte count of the items still to redraw, once per call and
 *      once per redraw pass.  Without non-units that is one small kernel and that readback on top of sample -> invert -> public key.
 *   host form: every output is optional except flags; packed_h [B][output_size][4] = packOutput(q - 1, N, h) (index.js:572-596, sizes
 *      from ntru_pack_params(q - 1, N, ...)) may be NULL. */
int ntru_keygen_workspace_bytes(int N, int64_t B, size_t *bytes);
int ntru_keygen_batch_dev(ntru_engine_t *eng, int N, int q, int p, int df, int dg, const uint32_t *key, uint64_t first_item, int max_tries,
                          int64_t B, void *d_work, int8_t *d_f, int8_t *d_g, uint16_t *d_fq, uint8_t *d_fp, uint16_t *d_h,
                          uint8_t *d_tries, uint8_t *d_flags);
int ntru_keygen_batch(ntru_engine_t *eng, int N, int q, int p, int df, int dg, const uint32_t *key, uint64_t first_item, int max_tries,
                      int64_t B, int8_t *f, int8_t *g, uint16_t *fq, uint8_t *fp, uint16_t *h, uint8_t *tries, uint8_t *flags,
                      uint64_t *packed_h);

/* generatePublicKeyH (index.js:72-79) for B keys: h[b] = remainder of ((p * fq[b]) mod q) * g[b] by 1 - x^N, mod q
 * (before trimPolynomial).  fq: mod-q inverse of f, g in {-1,0,1}; p*(q-1) must fit 16 bits.  Per-item operands on both
 * sides: one key per wavefront on the matrix cores (k_public_key_m) for 128 <= N <= 1024 and q <= 8192, the vector-ALU
 * product kernel otherwise.  [§8(f) #1, the part of key generation that is a product] */
int ntru_public_key_batch(ntru_engine_t *eng, int N, int q, int p, const uint16_t *fq, const int8_t *g, int64_t B,
                          uint16_t *h);
int ntru_public_key_batch_dev(ntru_engine_t *eng, int N, int q, int p, const uint16_t *d_fq, const int8_t *d_g,
                              int64_t B, uint16_t *d_h);

/* ---- verifyKeysInputs (index.js:141-197) for B independent key pairs (per-item operands).
 *      f, g [B][N] in {-1,0,1}; fq, h [B][N] in [0,q); fp [B][N] in [0,p).
 *      Three witnesses per item: fq*f mod q, fp*f mod p, (p*fq)*g mod q, each as quotient + remainder;
 *      flags[B] gets the NTRU_FLAG_* bits.  One key pair per wavefront; on the matrix cores where the note at the top
 *      of this file says so (k_verify_keys_m), otherwise on the ternary add path / the multiply-accumulate kernels. */
int ntru_verify_keys_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const int8_t *g,
                           const uint16_t *fq, const uint8_t *fp, const uint16_t *h, int64_t B,
                           uint16_t *quot_fq, uint16_t *rem_fq, uint8_t *quot_fp, uint8_t *rem_fp,
                           uint16_t *quot_h, uint16_t *rem_h, uint8_t *flags);
int ntru_verify_keys_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const int8_t *d_g,
                               const uint16_t *d_fq, const uint8_t *d_fp, const uint16_t *d_h, int64_t B,
                               uint16_t *d_quot_fq, uint16_t *d_rem_fq, uint8_t *d_quot_fp, uint8_t *d_rem_fp,
                               uint16_t *d_quot_h, uint16_t *d_rem_h, uint8_t *d_flags);

/* ---- pinned host memory.  Buffers from ntru_host_alloc are page-locked: the host-pointer entry points below DMA
 *      straight from / to them (any other host memory is staged through the engine's own pinned arenas, which costs a
 *      CPU copy per byte).  The N-API addon hands them to JavaScript as TypedArrays (allocUint8 / allocUint16). */
void *ntru_host_alloc(size_t bytes);
void ntru_host_free(void *p);

/* ---- several devices in one process (contiguous batch shards, no exchange between devices).  One engine
 *      per listed device id (an id may be listed more than once: every entry is its own engine with its own streams), one
 *      host thread per engine for the duration of a call; device g gets the items [g B / G, (g + 1) B / G).  Host pointers,
 *      same meaning as the single-device entry points above; on failure the message names the shard.  (bench.py's multi-GPU
 *      mode is one process per GPU under torchrun instead; this is for a host that owns all GPUs of a node, e.g. Node.js.) */
typedef struct ntru_multi ntru_multi_t;
int ntru_multi_create(const int *device_ids, int n_dev, ntru_multi_t **out);
void ntru_multi_destroy(ntru_multi_t *m);
int ntru_multi_engines(const ntru_multi_t *m);
/* ntru_engine_set_lift on every engine of `m` (a NULL `m`, then an unknown mode: NTRU_ERR_ARG, nothing changed). */
int ntru_multi_set_lift(ntru_multi_t *m, int lift);
int ntru_multi_encrypt_batch(ntru_multi_t *m, int N, int q, const uint16_t *h, const uint8_t *r, const uint8_t *mm, int64_t B,
                             uint16_t *e, uint16_t *quotE);
int ntru_multi_decrypt_batch(ntru_multi_t *m, int N, int q, int p, const int8_t *f, const uint8_t *fp, const uint16_t *e,
                             int64_t B, uint8_t *value, uint16_t *quot1, uint16_t *rem1, uint8_t *quot2);
int ntru_multi_verify_keys_batch(ntru_multi_t *m, int N, int q, int p, const int8_t *f, const int8_t *g, const uint16_t *fq,
                                 const uint8_t *fp, const uint16_t *h, int64_t B, uint16_t *quot_fq, uint16_t *rem_fq,
                                 uint8_t *quot_fp, uint8_t *rem_fp, uint16_t *quot_h, uint16_t *rem_h, uint8_t *flags);
int ntru_multi_polymul_split(ntru_multi_t *m, int N, int mod, const uint16_t *a, const uint16_t *b, int64_t B, uint16_t *quot,
                             uint16_t *rem);
int ntru_multi_invert_key_batch(ntru_multi_t *m, int N, int q, int p, const int8_t *f, int64_t B, uint16_t *fq, uint8_t *fp,
                                uint8_t *flags);
int ntru_multi_public_key_batch(ntru_multi_t *m, int N, int q, int p, const uint16_t *fq, const int8_t *g, int64_t B,
                                uint16_t *h);

/* ---- generic, reference-faithful family (ntru_generic.hip): the reference's own algorithms on int64 coefficients, for
 *      what the fast kernels do not cover -- moduli above 65536 (multiplyPolynomials(a, b, 2^20), test/circuits.test.js:72),
 *      arbitrary divisors (dividePolynomials, index.js:358-401, e.g. test/circuits.test.js:165-170), and the stand-alone
 *      extendedEuclideanAlgorithm (index.js:425-459) / polyInv (index.js:491-514) incl. their behaviour on non-units.
 *      a: [B][la], b: [B][lb] signed, possibly unreduced coefficients, |x| <= 2^26; 1 <= mod <= 2^26 (every product the
 *      reference forms then stays exact in a JS double).  Every item of a batch has the same operand lengths la, lb --
 *      lengths matter to the reference (a.length, `r0.length !== 1`), so callers must not pad.  Result rows have a pitch of
 *      ntru_generic_capacity(la, lb) elements; *_len[b] is the length of the (trimmed) result array the reference returns.
 *      status[b]: 0, or the NTRU_GENERIC_* code of the error the reference throws for item b (its results are then empty).
 *      Host pointers; one item per wavefront; a latency path, not a throughput path. */
#define NTRU_GENERIC_DIV_BY_ZERO 1  /* "Cannot divide by zero polynomial."  (index.js:360) */
#define NTRU_GENERIC_NO_INVERSE 2   /* "No inverse exists for division."    (index.js:378) */
#define NTRU_GENERIC_INVALID_GCD 3  /* "invalid_gcd"                        (index.js:452) */
#define NTRU_GENERIC_CAPACITY 4     /* internal: a result outgrew the work area (never expected) */
int ntru_generic_capacity(int la, int lb);
/* multiplyPolynomials(a, b, mod): out[b] = the linear product, coefficients in [0, mod), trimmed ([0] when la or lb is 0). */
int ntru_generic_multiply(ntru_engine_t *eng, int la, int lb, int64_t mod, const int64_t *a, const int64_t *b, int64_t B,
                          int64_t *out, int32_t *out_len);
/* dividePolynomials(a, b, mod) -> { quotient, remainder } exactly as index.js:358-401 computes them. */
int ntru_generic_divide(ntru_engine_t *eng, int la, int lb, int64_t mod, const int64_t *a, const int64_t *b, int64_t B,
                        int64_t *quot, int32_t *quot_len, int64_t *rem, int32_t *rem_len, uint8_t *status);
/* extendedEuclideanAlgorithm(a, b, mod) -> { gcd, inverse } (index.js:425-459). */
int ntru_generic_eea(ntru_engine_t *eng, int la, int lb, int64_t mod, const int64_t *a, const int64_t *b, int64_t B,
                     int64_t *gcd, int32_t *gcd_len, int64_t *inverse, int32_t *inverse_len, uint8_t *status);
/* polyInv(a, polyI, mod) (index.js:491-514): EEA modulo 2 + log2(mod) - 1 Newton rounds when mod is a power of two,
 * plain EEA otherwise. */
int ntru_generic_poly_inv(ntru_engine_t *eng, int la, int lb, int64_t mod, const int64_t *a, const int64_t *poly_i,
                          int64_t B, int64_t *inverse, int32_t *inverse_len, uint8_t *status);

/* ---- BN254 field-element packing: packOutput / unpackInput (index.js:572-620), the wire format of the circuits'
 *      CombineArray / UnpackArray (circuits/ntru.circom:258-306).  bits = floor(log2(max_val)+1) per value,
 *      per_output = floor(252/bits) values per field element, arr_len / output_size as index.js:575-580.
 *      A field element is four little-endian uint64 limbs.  1 <= max_val <= 65535.
 *      pack:   data [B][data_len] -> out [B][output_size][4];   out[b][o] = sum_j data[b][o*per+j] << (j*bits)
 *      unpack: in [B][packed_size][4] -> out [B][packed_size*per], per = floor(packed_bits/bits) (trimming is host glue) */
int ntru_pack_params(int max_val, int data_len, int *bits, int *per_output, int *arr_len, int *output_size);
int ntru_pack_batch(ntru_engine_t *eng, int max_val, int data_len, const uint16_t *data, int64_t B, uint64_t *out);
int ntru_pack_batch_dev(ntru_engine_t *eng, int max_val, int data_len, const uint16_t *d_data, int64_t B, uint64_t *d_out);
/* packOutput of an array of BYTES (values <= 255: decryptBits' value and quotient2, r, m) without widening it to uint16 first. */
int ntru_pack_bytes_batch_dev(ntru_engine_t *eng, int max_val, int data_len, const uint8_t *d_data, int64_t B, uint64_t *d_out);
/* decryptBits (index.js:111-140) + packOutput(p - 1, N, value) (index.js:572-596) of its result, value-only mode, device pointers:
 * d_packed [B][output_size][4] (sizes from ntru_pack_params(p - 1, N, ...)).  Where the matrix-core decrypt applies (shared key, p == 3,
 * q <= 8192, N <= 1024, d_packed 16-byte aligned) AND the kernel's 2-bit image of the values fits behind its mod-p tables in the LDS
 * (it does from N of about 100 up; every BASELINE size) this is ONE kernel -- the field elements come straight out of the second
 * product's epilogue and d_value may be NULL (nothing but the packed rows is written); elsewhere it is decrypt + pack, d_value is
 * needed as the intermediate and a NULL d_value is NTRU_ERR_ARG. */
int ntru_decrypt_pack_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                const uint16_t *d_e, int64_t B, uint8_t *d_value, uint64_t *d_packed);
/* encryptBits (index.js:87-110) + packOutput(q - 1, N, e) (index.js:572-596) of its result, device pointers: d_packed
 * [B][output_size][4] (sizes from ntru_pack_params(q - 1, N, ...)).  With d_e == NULL and where the row-image matrix kernel applies
 * (shared key, q in {2048, 4096, 8192}, N <= 1024, d_packed 16-byte aligned) this is ONE kernel that writes nothing but the packed
 * rows (32 output_size bytes per ciphertext instead of 2 N + 32 output_size); with d_e != NULL, or elsewhere, it is encrypt (e only)
 * + pack, and d_e is needed. */
int ntru_encrypt_pack_batch_dev(ntru_engine_t *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, const uint8_t *d_m,
                                int64_t B, uint16_t *d_e, uint64_t *d_packed);
int ntru_unpack_batch(ntru_engine_t *eng, int max_val, int packed_bits, const uint64_t *in, int packed_size, int64_t B,
                      uint16_t *out);
int ntru_unpack_batch_dev(ntru_engine_t *eng, int max_val, int packed_bits, const uint64_t *d_in, int packed_size,
                          int64_t B, uint16_t *d_out);

/* ---- witness checks: does a witness satisfy the reference's circuit (circuits/ntru.circom with circomlib 2.0.5 LessThan, LessEqThan,
 *      IsEqual, IsZero, Num2Bits)?  VerifyEncrypt(q, nq, N), VerifyDecrypt(q, nq, p, np, N), VerifyInverse(M, n, N) -- the witnesses
 *      of encryptBits, decryptBits and verifyKeysInputs()[fq | fp | h] (index.js:87-197).  Every operand is per item, every array dense
 *      uint16_t: [B][N] for the N-long signals, [B][N+1] for the quotients and remainders; every entry must be below 65536.
 *      The constraint system is evaluated exactly, range checks included (Modulus's ltP / gteZeroY / ltQ, decrypt's LessThan(nq)).
 *      flags[b] = 0: item b is accepted; else the OR of the NTRU_CHECK_* bits below, VerifyDecrypt's second stage (mod p) shifted
 *      left by 3.  Domain: 2 <= N <= NTRU_MAX_N; 2 <= q, M, p <= 65536; q even for VerifyDecrypt; 1 <= nq, np, n <= 252; anything
 *      else is NTRU_ERR_ARG, checked on the host before the engine.  One item per wavefront (k_check_encrypt / _decrypt / _inverse). */
#define NTRU_CHECK_EQ 1     /* some a_k differs from the reduced P_k of VerifyDividePolynomials */
#define NTRU_CHECK_TAIL 2   /* a reduced P_{2N-1} or P_{2N} is nonzero */
#define NTRU_CHECK_RANGE 4  /* some Modulus or LessThan range check of the stage fails */
int ntru_check_encrypt_batch(ntru_engine_t *eng, int N, int q, int nq, const uint16_t *r, const uint16_t *m, const uint16_t *h,
                             const uint16_t *quotE, const uint16_t *remE, int64_t B, uint8_t *flags);
int ntru_check_encrypt_batch_dev(ntru_engine_t *eng, int N, int q, int nq, const uint16_t *d_r, const uint16_t *d_m,
                                 const uint16_t *d_h, const uint16_t *d_quotE, const uint16_t *d_remE, int64_t B, uint8_t *d_flags);
int ntru_check_decrypt_batch(ntru_engine_t *eng, int N, int q, int nq, int p, int np, const uint16_t *f, const uint16_t *fp,
                             const uint16_t *e, const uint16_t *quot1, const uint16_t *rem1, const uint16_t *quot2,
                             const uint16_t *rem2, int64_t B, uint8_t *flags);
int ntru_check_decrypt_batch_dev(ntru_engine_t *eng, int N, int q, int nq, int p, int np, const uint16_t *d_f, const uint16_t *d_fp,
                                 const uint16_t *d_e, const uint16_t *d_quot1, const uint16_t *d_rem1, const uint16_t *d_quot2,
                                 const uint16_t *d_rem2, int64_t B, uint8_t *d_flags);
int ntru_check_inverse_batch(ntru_engine_t *eng, int N, int M, int n, const uint16_t *f, const uint16_t *fq, const uint16_t *quotI,
                             const uint16_t *remI, int64_t B, uint8_t *flags);
int ntru_check_inverse_batch_dev(ntru_engine_t *eng, int N, int M, int n, const uint16_t *d_f, const uint16_t *d_fq,
                                 const uint16_t *d_quotI, const uint16_t *d_remI, int64_t B, uint8_t *d_flags);

/* ---- re-randomising and shuffling ciphertexts under the shared public key h: encryptBits (index.js:87-110) with an existing
 *      ciphertext in the place of m -- addPolynomials(e, multiplyPolynomials(r, h, q), q), then dividePolynomials(., I, q)
 *      (index.js:90-92).  VerifyEncrypt puts no range constraint on m (circuits/ntru.circom:188-208), so
 *      {r, m: the old row, h, quotientE, remainderE} is a valid witness and ntru_check_encrypt_batch accepts it.
 *      For output row i, s = src ? src[i] : i:
 *        e_out[i] = remainder and quotE[i] = quotient mod q of (r[i] * h + e_in[s]) mod q split by 1 - x^N,
 *      exactly what ntru_encrypt_batch writes for (h, r[i], m) with m the 16-bit row e_in[s]:
 *        e_out[i] = (Enc(0; r[i]) + e_in[s]) mod q, and quotE[i] is that of Enc(0; r[i]).
 *      e_in [B_in][N]: any uint16_t value, reduced mod q.  src [B] (DEVICE memory in the _dev form) is a general gather: repeats are
 *      allowed and B may differ from B_in; src == NULL needs B <= B_in.  quotE may be NULL.  (N, q), h and r as for
 *      ntru_encrypt_batch, with the same choice of kernels (ntru_engine_set_kernel_path): where the matrix-core encrypt applies this
 *      is ONE kernel (k_reencrypt_md / k_reencrypt_m: r in, the old row in, e and the quotient out, 7 N bytes per row); elsewhere the
 *      vector-ALU encrypt of a zero message followed by one add kernel, with the same bytes.
 *      NTRU_ERR_ARG before anything is launched: a NULL buffer, a negative size, src == NULL with B > B_in, e_in and e_out ranges
 *      that overlap while src is given (with src == NULL, e_out == e_in -- in place -- is allowed), and in the host form an index
 *      outside [0, B_in).  In the _dev form an index outside [0, B_in) is not an error: the kernels never read outside
 *      e_in[0 .. B_in) -- to the dword: a row that is read is read in whole dwords, so up to 2 bytes next to an e_in that is not
 *      4-byte aligned share an access with it -- and such a row is not read at all: it takes an all-zero addend, so its result is
 *      Enc(0; r[i]). */
int ntru_reencrypt_batch_dev(ntru_engine_t *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, const uint16_t *d_e_in,
                             int64_t B_in, const int64_t *d_src, int64_t B, uint16_t *d_e_out, uint16_t *d_quotE);
int ntru_reencrypt_batch(ntru_engine_t *eng, int N, int q, const uint16_t *h, const uint8_t *r, const uint16_t *e_in, int64_t B_in,
                         const int64_t *src, int64_t B, uint16_t *e_out, uint16_t *quotE);

/* ---- drawing the mix order: the permutation of a mix step from the same kind of ChaCha20 stream as r and the keys, made by a
 *      stable sort on the device, and a whole mix step from a key (permutation.hip).
 *      The permutation of B items under `key` (8 words, a HOST pointer in every form, as for ntru_sample_ternary) and perm_id:
 *        k_i    = w[2 j] | (uint64_t)w[2 j + 1] << 32 with j = i mod 8, where w[0..15] is the output of the RFC 8439 ChaCha20 block
 *                 function under `key` with block counter floor(i / 8) and nonce (perm_id_lo, perm_id_hi, NTRU_PERM_NONCE2).
 *                 NTRU_PERM_NONCE2 ("PERM") differs from the sampler's 0x4e545255 ("NTRU"), so a permutation never shares a block
 *                 with a draw of r or of a key under the same key.  Always 20 rounds: ntru_engine_set_sampler_rounds does not apply
 *                 (as for ntru_keygen_batch).
 *        src    = the stable ascending argsort of k: src[j] is the index whose key has rank j; equal keys keep index order.
 *        dst    = its inverse: dst[src[j]] = j.
 *      Any host replays it with a ChaCha20 implementation and a stable sort.  The order is uniform up to ties: two of the B keys
 *      collide with probability below B^2 / 2^65 (about 2^-25 at B = 2^20), and a tie resolves by index.
 *      0 <= B <= NTRU_PERM_MAX_B; B == 0 is NTRU_OK with nothing launched.
 *      ntru_argsort_keys_dev is the sort by itself: d_order [B] = the stable ascending argsort of ANY device keys d_keys [B], which
 *      are not modified; the two ranges must not overlap.  Eight passes of one byte, per pass a per-tile digit histogram
 *      (k_perm_hist), exclusive offsets over digit x tile (k_perm_offsets) and a scatter that ranks every key inside its tile in
 *      key order (k_perm_scatter); positions come from prefix sums only -- no global atomic -- and every dependency between
 *      workgroups is a kernel boundary.  The temporaries (24 B per key + 1 KiB per 1024 keys) come from the engine's scratch buffer.
 *      ntru_draw_permutation[_dev]: d_dst may be NULL; d_src may be NULL only if d_dst is not.  The host form brings only src / dst
 *      down.
 *      ntru_mix_batch_dev is one mix step from a key, enqueued on the engine's stream as
 *        ntru_sample_ternary_dev(N, n1, n2, p - 1, key, first_item, B) into d_r,
 *        the permutation (key, perm_id) into d_src,
 *        ntru_reencrypt_batch_dev(N, q, d_h, d_r, d_e_in, B, d_src, B, d_e_out, d_quotE).
 *      d_r [B][N] uint8_t and d_src [B] int64_t are outputs the caller owns and must supply (the prover needs both for the witness:
 *      {r, m: e_in[src[i]], h, quotientE, remainderE}); d_quotE may be NULL; d_e_out must not overlap d_e_in.  The sampler honours
 *      ntru_engine_set_sampler_rounds and the re-encrypt the kernel path, as everywhere.
 *      ntru_mix_batch is the host-pointer form: the permutation is drawn on the device and brought down, the rows e_in[src[o ..]]
 *      are gathered while the staging buffer of a chunk is filled (as ntru_reencrypt_batch does), r is sampled on the device per
 *      chunk from positions first_item + o .. -- it never goes up, and comes down only when r_out is given.  r_out, src_out and
 *      quotE may be NULL.
 *      NTRU_ERR_ARG with a message of its own, before the engine is looked at and before anything is launched: B < 0,
 *      B > NTRU_PERM_MAX_B, a NULL key, a NULL required buffer with B > 0, overlapping ranges where they are forbidden (keys / order,
 *      src / dst, e_in / e_out, and any two outputs of a mix call), and for the mix calls what ntru_sample_ternary refuses; then a
 *      NULL engine and what ntru_reencrypt_batch refuses. */
#define NTRU_PERM_NONCE2 0x5045524du
#define NTRU_PERM_MAX_B (1 << 24)
int ntru_argsort_keys_dev(ntru_engine_t *eng, const uint64_t *d_keys, int64_t B, int64_t *d_order);
int ntru_draw_permutation_dev(ntru_engine_t *eng, const uint32_t *key, uint64_t perm_id, int64_t B, int64_t *d_src, int64_t *d_dst);
int ntru_draw_permutation(ntru_engine_t *eng, const uint32_t *key, uint64_t perm_id, int64_t B, int64_t *src, int64_t *dst);
int ntru_mix_batch_dev(ntru_engine_t *eng, int N, int q, int p, const uint16_t *d_h, const uint32_t *key, uint64_t first_item, int n1,
                       int n2, uint64_t perm_id, const uint16_t *d_e_in, int64_t B, uint8_t *d_r, int64_t *d_src, uint16_t *d_e_out,
                       uint16_t *d_quotE);
int ntru_mix_batch(ntru_engine_t *eng, int N, int q, int p, const uint16_t *h, const uint32_t *key, uint64_t first_item, int n1, int n2,
                   uint64_t perm_id, const uint16_t *e_in, int64_t B, uint8_t *r_out, int64_t *src_out, uint16_t *e_out, uint16_t *quotE);

/* ---- auditing a mix: checking revealed re-encryption links (mix_audit.hip).  A mixer that opens a link names (index in, index out,
 *      r); link l of L holds when, coefficient by coefficient,
 *        e_out[o] == r[l] * h + e_in[i]   modulo (x^N - 1, q),   i = in_idx ? in_idx[l] : l,   o = out_idx ? out_idx[l] : l,
 *      both sides reduced mod q (a coefficient with q added still matches; q == 65536: raw equality).  This is what
 *      ntru_reencrypt_batch computes, compared against a row instead of stored: no quotient, 5 N bytes read per link, one written.
 *      r [L][N] uint8_t; in_idx, out_idx [L] int64_t (DEVICE memory in the _dev form; either may be NULL); e_in [B_in][N] and e_out
 *      [B_out][N] uint16_t, any value, may be the same array or overlap (both are only read); flags [L] uint8_t; n_bad one int64_t,
 *      SET to the number of links whose flag is not 0 (a device scalar in the _dev form; may be NULL).  Nothing is written to r, e_in
 *      or e_out.  flags[l] is 0 when the link holds, else
 *        NTRU_LINK_BAD_INDEX  i outside [0, B_in) or o outside [0, B_out): no row of that link is read.  A finding in BOTH forms, not
 *                             an argument error (here the host form differs from ntru_reencrypt_batch);
 *        NTRU_LINK_BAD_R      a byte of r[l] outside {0, 1, other}; or n1 >= 0 and the ones do not number n1; or n2 >= 0 and the
 *                             bytes equal to other do not number n2.  With other == 1 the two counts are of the same bytes: the ones
 *                             must number n1 + n2 when both are given, and are not counted when either is negative;
 *        NTRU_LINK_MISMATCH   some coefficient differs.  Reported only when neither other bit is set: a link with a bad index or a
 *                             bad r carries exactly those bits, and its product is never relied on.
 *      other is 1, 2 or 3 (p - 1; 2 for p = 3): the matrix planes carry 32 r without carries only for r <= 3.
 *      Where the matrix-core encrypt applies (64 <= N <= 1024, a power-of-two q <= 8192, kernel paths 0, 4 and 5) this is ONE kernel,
 *      k_linkcheck_md / k_linkcheck_m by the rule of k_reencrypt_md / _m: the encrypt body with the gathered e_in row as addend and
 *      a compare against the columns of e_out[o] in the place of the stores.  Elsewhere the vector-ALU encrypt of a zero message
 *      into the engine's scratch, at most 65536 links per pass (with the bytes of r outside the domain cleared first, so that it
 *      only ever sees its documented operands), then k_compare_links.
 *      NTRU_ERR_ARG before anything is launched: a NULL required buffer with L > 0, a negative size, other outside 1 .. 3,
 *      n1 + n2 > N, flags (or n_bad) overlapping an input, and what every batch call refuses (a NULL engine, an unsupported (N, q)).
 *      L == 0 launches nothing and sets n_bad to 0 when it is given.
 *      _dev: enqueued on the engine's stream, no synchronisation, nothing allocated per call.  Host form: the links run through the
 *      chunked pipeline, both rows of a link gathered on the host while a chunk's staging buffer is filled. */
#define NTRU_LINK_BAD_INDEX 1
#define NTRU_LINK_BAD_R 2
#define NTRU_LINK_MISMATCH 4
int ntru_check_links_batch_dev(ntru_engine_t *eng, int N, int q, int other, int n1, int n2, const uint16_t *d_h, const uint8_t *d_r,
                               const uint16_t *d_e_in, int64_t B_in, const int64_t *d_in_idx, const uint16_t *d_e_out, int64_t B_out,
                               const int64_t *d_out_idx, int64_t L, uint8_t *d_flags, int64_t *d_n_bad);
int ntru_check_links_batch(ntru_engine_t *eng, int N, int q, int other, int n1, int n2, const uint16_t *h, const uint8_t *r,
                           const uint16_t *e_in, int64_t B_in, const int64_t *in_idx, const uint16_t *e_out, int64_t B_out,
                           const int64_t *out_idx, int64_t L, uint8_t *flags, int64_t *n_bad);

/* ---- removing duplicates: which rows of a batch repeat an earlier row, of the batch or of a set accepted before (dedup_rows.hip).  A
 *      replayed ciphertext counts twice in a tally and comes out of a mix as a recognisable pair, so intake rejects it first.
 *      Two rows are EQUAL MODULO mod when row_a[k] % mod == row_b[k] % mod for every k < N; 2 <= N <= NTRU_MAX_N, 2 <= mod <= 65536,
 *      a power of two or not (mod == 65536: raw equality).  A row with mod added to a coefficient is therefore a duplicate.  Packed
 *      rows ([rows][output_size][4] uint64_t, geometry from ntru_pack_params(mod - 1, N, ...), "packed ciphertexts" above) compare by
 *      their N fields, each reduced modulo mod: fields with index >= N and the bits of an element above per * bits are ignored, and a
 *      raw field >= mod counts as its remainder.  A homomorphically re-randomised copy is a different row: out of scope here.
 *      The S rows of `prior` (accepted in earlier batches; S may be 0 with prior NULL) take the indices 0 .. S - 1, the B new rows
 *      S .. S + B - 1; both sets in the same format; S + B <= NTRU_DEDUP_MAX_ROWS.  Outputs, for the B new rows only:
 *        first  [B] int64_t  first[b] = the smallest combined index of a row equal to new row b; row b is a first occurrence exactly
 *                            when first[b] == S + b (prior rows may repeat one another: the smallest index is named);
 *        unique [B] int64_t  the batch-local indices b of the first occurrences, ascending; only the first count[0] entries are
 *                            written, nothing behind them;
 *        count  [1] int64_t  SET to the number of first occurrences.
 *      first may be NULL, unique may be NULL, count is required.  Positions come from prefix sums only, never from the arrival order
 *      of an atomic: the bytes are the same for any launch shape, salt and fingerprint width.
 *      salt keys the 64-bit row fingerprint that is sorted (ntru_argsort_keys_dev): a submitter who does not know it cannot craft
 *      fingerprint collisions; results do not depend on it.  fingerprint_bits (0 .. 64; 64 in production) keeps only that many low
 *      bits: fewer cost time (rows with equal fingerprints are compared in full, a first occurrence against every earlier distinct
 *      row of its fingerprint) and never change a byte of the result; 0 makes every row collide.  Equality is always decided on
 *      the full reduced rows, never on the fingerprint, whose function is internal.
 *      _dev: enqueued on the engine's stream without synchronising, nothing is allocated; d_work is a caller-owned device workspace of
 *      ntru_dedup_workspace_bytes(N, S + B) bytes (fingerprints, sorted order, flags; monotone in the row count, 256-byte granular),
 *      as ntru_keygen_workspace_bytes.  The sort takes the engine's scratch buffer for itself.
 *      Host forms: the S + B rows, the workspace and the outputs live in the engine's resident buffer for the call; the rows go up
 *      through the staging pipeline; count, first and the count[0]-entry prefix of unique come down.
 *      NTRU_ERR_ARG with a message of its own, before the engine is looked at: B < 0 or S < 0, S + B > NTRU_DEDUP_MAX_ROWS,
 *      fingerprint_bits outside 0 .. 64, N or mod out of range, a NULL count, a NULL required buffer with B > 0, S > 0 with a NULL
 *      prior, overlapping outputs (with one another, the inputs or the workspace); then a NULL engine.  B == 0 sets count[0] = 0 and
 *      launches nothing else. */
#define NTRU_DEDUP_MAX_ROWS NTRU_PERM_MAX_B                      /* S + B */
int ntru_dedup_workspace_bytes(int N, int64_t total_rows, size_t *bytes);
int ntru_dedup_rows_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_prior, int64_t S, const uint16_t *d_rows, int64_t B,
                        uint64_t salt, int fingerprint_bits, void *d_work, int64_t *d_first, int64_t *d_unique, int64_t *d_count);
int ntru_dedup_packed_dev(ntru_engine_t *eng, int N, int mod, const uint64_t *d_prior, int64_t S, const uint64_t *d_packed, int64_t B,
                          uint64_t salt, int fingerprint_bits, void *d_work, int64_t *d_first, int64_t *d_unique, int64_t *d_count);
int ntru_dedup_rows(ntru_engine_t *eng, int N, int mod, const uint16_t *prior, int64_t S, const uint16_t *rows, int64_t B, uint64_t salt,
                    int fingerprint_bits, int64_t *first, int64_t *unique, int64_t *count);
int ntru_dedup_packed(ntru_engine_t *eng, int N, int mod, const uint64_t *prior, int64_t S, const uint64_t *packed, int64_t B,
                      uint64_t salt, int fingerprint_bits, int64_t *first, int64_t *unique, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* NTRU_ENGINE_H */
