// matrix_reencrypt.hip -- MI355X (gfx950): re-randomising and shuffling ciphertexts under the shared public key, encryptBits
// (index.js:87-110) with an existing ciphertext row in the place of m: e_out[i] = (r[i] * h + e_in[src[i]]) mod q split by 1 - x^N.
// VerifyEncrypt does not constrain the range of m (circuits/ntru.circom:188-208), so the old row is a valid witness value.
// k_reencrypt_m / k_reencrypt_md are the body of k_encrypt_m / k_encrypt_md (matrix_encrypt_body.h) with a gathered 16-bit row as the
// epilogue's addend instead of the byte image of m: r in, the old row in, e and the quotient out -- 7 N bytes per row against about
// 16 N for the composition gather + encrypt of a zero message + add.  Outside the matrix path's range (q > 8192, N > 1024, kernel
// paths 1-3) the vector-ALU encrypt runs on a zero message from the engine's scratch buffer and k_add_gathered_rows adds the rows:
// the same bytes.  The entry points, _dev and host-pointer form, are at the end of this file.
#include <algorithm>
#include <vector>

#include "matrix_encrypt_body.h"

typedef AddGatherRows16 ReAdd;
constexpr size_t RE_STAGE_BYTES = (size_t)WAVES_PER_BLOCK * 32 * ADD_ROW_PITCH;    // every wave's staged addend columns

// e_out and e_in are not __restrict__: with src == NULL they may be the same array (every element is staged by the wave that writes
// it, before it writes it).
__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_reencrypt_m(MGeom g, u32 q, const u16 *__restrict__ h,
                                                               const uint8_t *__restrict__ r, const u16 *e_in, long B_in,
                                                               const long *__restrict__ src, long B, u16 *e_out, u16 *quotE) {
  encrypt_m_body<4, false, ReAdd>(g, q, h, r, nullptr, B, e_out, quotE, ReAdd{e_in, B_in, src});
}

__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_reencrypt_md(MGeom g, u32 q, const u16 *__restrict__ h,
                                                                const uint8_t *__restrict__ r, const u16 *e_in, long B_in,
                                                                const long *__restrict__ src, long B, u16 *e_out, u16 *quotE) {
  encrypt_m_body<4, true, ReAdd>(g, q, h, r, nullptr, B, e_out, quotE, ReAdd{e_in, B_in, src});
}

// e_out[first + i] = (enc0[i] + e_in[s]) mod q for the n rows of a pass, s = src ? src[first + i] : first + i; a row whose s lies
// outside [0, B_in) adds nothing (and reads nothing).  One element per thread.
__global__ void __launch_bounds__(256) k_add_gathered_rows(int N, u32 q, const u16 *__restrict__ enc0, const u16 *e_in, long B_in,
                                                           const long *__restrict__ src, long first, long n, u16 *e_out) {
  const long total = n * N;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long i = idx / N, row = first + i;
    const int c = (int)(idx - i * N);
    const long s = src ? src[row] : row;
    u32 a = 0;
    if ((unsigned long)s < (unsigned long)B_in) a = e_in[s * N + c];
    e_out[row * N + c] = (u16)(((u32)enc0[idx] + a) & (q - 1));
  }
}

namespace {

constexpr int64_t RE_PASS = 65536;       // rows per pass of the vector-ALU route (bounds the scratch it takes)

// Kernel paths as for ntru_launch_encrypt_matrix: 0 = auto and 5 -> k_reencrypt_md where a row of r fits one direct-to-LDS
// instruction, else k_reencrypt_m; 4 -> k_reencrypt_m.  LDS: the two key arrays, the r stage, the 256-byte row table and the four
// waves' staged addend columns: 74 KB at N = 821, two workgroups per CU up to N = 928.
int launch_reencrypt_matrix(ntru_engine *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, const uint16_t *d_e_in, int64_t B_in,
                            const int64_t *d_src, int64_t B, uint16_t *d_e_out, uint16_t *d_quotE) {
  MGeom mg;
  if (!make_mgeom(eng, N, q, N, &mg)) return NTRU_NOT_TAKEN;
  const size_t lds = (size_t)32 * mg.tpitch + (size_t)32 * mg.pitchA + 256 + RE_STAGE_BYTES + 16;
  if (lds > 160 * 1024) return NTRU_NOT_TAKEN;
  const long nrb = (long)((B + 31) / 32);
  const bool rows_dword_aligned = (N & 3) == 0 && ((uintptr_t)d_r & 3) == 0;
  const bool md = eng->path != 4 && (N + 3 <= 1024 || (rows_dword_aligned && N <= 1024));
  note_kernel(eng, md ? "k_reencrypt_md" : "k_reencrypt_m");
  return launch_resident(eng, md ? k_reencrypt_md : k_reencrypt_m, nrb, BLOCK_THREADS, lds, mg, (u32)q, d_h, d_r, d_e_in, (long)B_in,
                         (const long *)d_src, (long)B, d_e_out, d_quotE);
}

// Enc(0; r) of a pass into scratch (e_out may be e_in: nothing is written to it before the add has read the old row), then the add.
int launch_reencrypt_valu(ntru_engine *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, const uint16_t *d_e_in, int64_t B_in,
                          const int64_t *d_src, int64_t B, uint16_t *d_e_out, uint16_t *d_quotE) {
  const int64_t pass = std::min<int64_t>(B, RE_PASS);
  Carve c;
  const size_t at_zero = c.take((size_t)pass * N), at_enc0 = c.total;
  ScratchHold hold(eng, at_enc0 + (size_t)pass * N * 2);          // (the last array is not rounded up)
  if (hold.rc) return hold.rc;
  uint8_t *d_zero = (uint8_t *)hold.p + at_zero;
  uint16_t *d_enc0 = (uint16_t *)(hold.p + at_enc0);
  HIP_TRY(hipMemsetAsync(d_zero, 0, (size_t)pass * N, eng->stream));
  const int rc = for_each_pass(B, RE_PASS, [&](int64_t o, int64_t n) -> int {
    if (int rc = ntru_launch_encrypt_valu(eng, N, q, d_h, d_r + o * N, d_zero, n, d_enc0, rows_at(d_quotE, o * N))) return rc;
    hipLaunchKernelGGL(k_add_gathered_rows, elementwise_grid(eng, (long)n * N), dim3(256), 0, eng->stream, N, (u32)q, d_enc0, d_e_in,
                       (long)B_in, (const long *)d_src, (long)o, (long)n, d_e_out);
    HIP_TRY(hipGetLastError());
    return NTRU_OK;
  });
  if (rc) return rc;
  note_kernel(eng, "k_add_gathered_rows");
  return NTRU_OK;
}

// The checks both forms share; *done: nothing to do (B == 0).
int check_reencrypt(ntru_engine *eng, int N, int q, const void *h, const void *r, const uint16_t *e_in, int64_t B_in, const int64_t *src,
                    int64_t B, const uint16_t *e_out, bool *done) {
  *done = false;
  if (int rc = ntru_check_common(eng, N, q, B)) return rc;
  if (B_in < 0) return fail(NTRU_ERR_ARG, "ntru_reencrypt_batch: negative input row count");
  if (!src && B > B_in) return fail(NTRU_ERR_ARG, "ntru_reencrypt_batch: without src, B must not exceed B_in");
  if (B == 0) { *done = true; return NTRU_OK; }
  if (!h || !r || !e_in || !e_out) return fail(NTRU_ERR_ARG, "ntru_reencrypt_batch: NULL buffer");
  if (ntru_ranges_overlap(e_in, (size_t)B_in * N * 2, e_out, (size_t)B * N * 2) && (src || e_in != e_out))
    return fail(NTRU_ERR_ARG, "ntru_reencrypt_batch: e_in and e_out overlap (only src == NULL with e_out == e_in works in place)");
  return NTRU_OK;
}

}  // namespace

extern "C" int ntru_reencrypt_batch_dev(ntru_engine_t *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, const uint16_t *d_e_in,
                                        int64_t B_in, const int64_t *d_src, int64_t B, uint16_t *d_e_out, uint16_t *d_quotE) {
  bool done;
  if (int rc = check_reencrypt(eng, N, q, d_h, d_r, d_e_in, B_in, d_src, B, d_e_out, &done)) return rc;
  if (done) return NTRU_OK;
  HIP_TRY(hipSetDevice(eng->device));
  const int rc = launch_reencrypt_matrix(eng, N, q, d_h, d_r, d_e_in, B_in, d_src, B, d_e_out, d_quotE);
  if (rc != NTRU_NOT_TAKEN) return rc;
  return launch_reencrypt_valu(eng, N, q, d_h, d_r, d_e_in, B_in, d_src, B, d_e_out, d_quotE);
}

// The host form gathers the rows while it fills the staging buffers (one chunk's rows at a time), so the device sees src == NULL.
// r == NULL (ntru_mix_batch, permutation.hip): row i of r is drawn on the device, chunk by chunk, as row 0 of
// ntru_sample_ternary_dev(N, n1, n2, other, key, first_item + i, 1); it never goes up and comes down only when draw->r_out is given.
int ntru_reencrypt_host(ntru_engine *eng, int N, int q, const uint16_t *h, const uint8_t *r, const ReencryptDraw *draw, const uint16_t *e_in,
                        int64_t B_in, const int64_t *src, int64_t B, uint16_t *e_out, uint16_t *quotE) {
  bool done;
  if (int rc = check_reencrypt(eng, N, q, h, r ? (const void *)r : (const void *)draw, e_in, B_in, src, B, e_out, &done)) return rc;
  if (done) return NTRU_OK;
  if (src)
    for (int64_t i = 0; i < B; i++)
      if (src[i] < 0 || src[i] >= B_in)
        return fail(NTRU_ERR_ARG, "ntru_reencrypt_batch: src[" + std::to_string(i) + "] = " + std::to_string(src[i]) + " is outside [0, B_in)");
  const size_t row = (size_t)N * 2;
  const int64_t C = ntru_chunk_items(B);
  std::vector<uint16_t> gathered;
  if (src) gathered.resize((size_t)std::min(C, B) * N);
  for (int64_t o = 0; o < B; o += src ? C : B) {          // with src: one pipeline run per chunk, on the rows gathered for it
    const int64_t n = src ? std::min(C, B - o) : B;
    if (src)
      for (int64_t i = 0; i < n; i++) memcpy(gathered.data() + (size_t)i * N, e_in + (size_t)src[o + i] * N, row);
    Pipeline P(eng);
    const int ih = P.in(h, row, true);
    const int ir = r ? P.in(r + o * N, N) : (draw->r_out ? P.out(draw->r_out + o * N, N) : P.tmp(N));
    const int ie = P.in(src ? gathered.data() : e_in, row);
    const int io = P.out(e_out + o * N, row), iq = P.out(quotE ? quotE + o * N : nullptr, row);
    const int rc = P.run(n, C, [&](int64_t first, int64_t cnt, void **d) {
      if (!r)
        if (int rs = ntru_sample_ternary_dev(eng, N, draw->n1, draw->n2, draw->other, draw->key, draw->first_item + (uint64_t)(o + first), cnt,
                                             (uint8_t *)d[ir]))
          return rs;
      return ntru_reencrypt_batch_dev(eng, N, q, (const uint16_t *)d[ih], (const uint8_t *)d[ir], (const uint16_t *)d[ie], cnt, nullptr, cnt,
                                      (uint16_t *)d[io], (uint16_t *)d[iq]);
    });
    if (rc) return rc;
  }
  return NTRU_OK;
}

extern "C" int ntru_reencrypt_batch(ntru_engine_t *eng, int N, int q, const uint16_t *h, const uint8_t *r, const uint16_t *e_in,
                                    int64_t B_in, const int64_t *src, int64_t B, uint16_t *e_out, uint16_t *quotE) {
  return ntru_reencrypt_host(eng, N, q, h, r, nullptr, e_in, B_in, src, B, e_out, quotE);
}
